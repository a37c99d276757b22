"""The actor's one-launch trunk section (hip/actor_section.hip.inc,
docs/ACTOR_SECTION.md): pool and both residual blocks with the image resident
in LDS.

Its arithmetic is fixed to that of the route it replaces, so every value
comparison here is `torch.equal`, on random bf16 data: against the pool kernel
followed by `ResidualBlock.forward_fused` twice (two MFMA launches per block)
for the kernel alone, against the fp64 integer reference and the flag-off
model for the whole trunk. The route test records the launches as
tests/test_trunk_routes.py does.
"""
import pytest
import torch
import torch.nn.functional as F

import trunk_refs as TR
from test_trunk_composed import BF16, build_model, int_case, int_inputs, int_ref, run_model
from test_trunk_routes import CONV1, PLAIN, Recorder, expected, run

gpu = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

SWITCHES = ("MOOLIB_AMD_NO_ACTOR_SECTION", "MOOLIB_AMD_CONV3_KERNEL", "MOOLIB_AMD_NO_FUSED_BIAS",
            "MOOLIB_AMD_NO_POOL_KERNEL")

# (N, H, W): one tile with a tail, odd sizes, a single row, more than one
# M-tile with a ragged tail (9 x 8 = 72 pixels)
SHAPES_ANY = [(1, 4, 4), (3, 5, 5), (2, 6, 7), (2, 1, 9), (1, 17, 16)]
# the section shapes; 84x84 at K=16 is the LDS-limit case (two 44x44x16 images)
SHAPES = {16: SHAPES_ANY + [(2, 84, 84)], 32: SHAPES_ANY + [(2, 42, 42), (2, 21, 21)]}
KERNEL_CASES = [(K, shape) for K in (16, 32) for shape in SHAPES[K]]


def make_blocks(K, g):
    """Two ResidualBlocks in bf16 on the GPU, biases around 0.1 so that every
    rounding point of the route matters, and a pending bias of that size."""
    from moolib_amd.models.atari import ResidualBlock

    blocks = []
    for _ in range(2):
        blk = ResidualBlock(K)
        with torch.no_grad():
            for conv in (blk.conv0, blk.conv1):
                conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / (9 * K)) ** 0.5)
                conv.bias.copy_(torch.randn(K, generator=g) * 0.1)
        blocks.append(blk.cuda().to(BF16))
    pending = (torch.randn(K, generator=g) * 0.1).to(BF16).cuda()
    return blocks[0], blocks[1], pending


def section_input(N, K, H, W, g):
    u = torch.randn(N, K, H, W, generator=g).to(BF16).cuda()
    return u.contiguous(memory_format=torch.channels_last)


def two_launch_route(u, pending, res0, res1, relu_out):
    """What the kernel replaces: pool kernel, two MFMA launches per block."""
    from moolib_amd.ops.pool import maxpool3x3s2

    with torch.no_grad():
        x = res1.forward_fused(res0.forward_fused(maxpool3x3s2(u), pending))
        return F.relu(x) if relu_out else x


@pytest.fixture
def default_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


# -------------------------------------------------------------------- kernel


@gpu
@requires_gpu
class TestKernel:
    @pytest.mark.parametrize("relu_out", [False, True], ids=["plain", "relu"])
    @pytest.mark.parametrize("with_pending", [False, True], ids=["nopending", "pending"])
    @pytest.mark.parametrize("K,shape", KERNEL_CASES, ids=lambda v: str(v).replace(" ", ""))
    def test_equals_two_launch_composition(self, K, shape, with_pending, relu_out,
                                           default_switches):
        from moolib_amd.ops import conv3x3 as c3

        N, H, W = shape
        g = torch.Generator().manual_seed(1000 * K + 100 * H + W)
        res0, res1, pending = make_blocks(K, g)
        pending = pending if with_pending else None
        u = section_input(N, K, H, W, g)
        assert c3.actor_section_available(u, K)
        want = two_launch_route(u, pending, res0, res1, relu_out)
        with torch.no_grad():
            got = c3.actor_section(u, pending, res0, res1, relu_out)
        assert got.shape == (N, K, (H + 1) // 2, (W + 1) // 2) and got.dtype == BF16
        assert got.is_contiguous(memory_format=torch.channels_last)
        assert want.abs().max().item() > 0.1          # not a comparison of zeros
        assert torch.equal(got, want), (got.float() - want.float()).abs().max().item()

    def test_rejections(self, default_switches):
        """A shape whose images exceed LDS, a wrong pack size and an input
        that is not channels_last raise before anything is launched."""
        from moolib_amd import _kernels
        from moolib_amd.ops import conv3x3 as c3

        g = torch.Generator().manual_seed(5)
        res0, res1, _ = make_blocks(32, g)
        convs = (res0.conv0, res0.conv1, res1.conv0, res1.conv1)
        packs = [c3.packed(c) for c in convs]
        biases = [c.bias.detach() for c in convs]
        small = section_input(1, 32, 6, 6, g)
        _kernels.actor_section_nhwc(small, None, packs, biases, False)   # the operands are fine

        big = section_input(1, 32, 84, 84, g)       # two 44x44x32 images: 242 KB
        assert not c3.actor_section_available(big, 32)
        with pytest.raises(RuntimeError, match="LDS"):
            _kernels.actor_section_nhwc(big, None, packs, biases, False)
        short = [packs[0], packs[1][:-8].contiguous(), packs[2], packs[3]]
        with pytest.raises(RuntimeError, match="w_packed"):
            _kernels.actor_section_nhwc(small, None, short, biases, False)
        res16 = make_blocks(16, g)[0]
        with pytest.raises(RuntimeError, match="w_packed"):   # a K=16 pack handed to K=32
            _kernels.actor_section_nhwc(
                small, None, [c3.packed(res16.conv0)] + packs[1:], biases, False)
        with pytest.raises(RuntimeError, match="bias"):
            _kernels.actor_section_nhwc(small, None, packs, biases[:3] + [biases[3][:16]], False)
        nchw = torch.randn(1, 32, 6, 6).to(BF16).cuda()
        with pytest.raises(RuntimeError, match="channels_last"):
            _kernels.actor_section_nhwc(nchw, None, packs, biases, False)
        torch.cuda.synchronize()


# --------------------------------------------------------------- whole trunk


def flagged(model, on=True):
    model.fused_actor_sections = on
    return model


@gpu
@requires_gpu
class TestTrunk:
    @pytest.mark.parametrize("mode", ["a", "b"])
    def test_integer_case(self, mode, default_switches):
        params, frames, _ = int_case()
        model = flagged(build_model(params, mode))
        got = run_model(model, mode, int_inputs(frames), no_grad=True)
        assert TR.bit_equal(got["trunk"], int_ref(mode, "kernel")["trunk"], BF16)

    @pytest.mark.parametrize("mode", ["a", "b"])
    def test_float_case_equals_flag_off(self, mode, default_switches):
        params, inputs, _, _ = TR.float_case(False)
        model = build_model(params, mode)
        off = run_model(model, mode, inputs, no_grad=True)
        on = run_model(flagged(model), mode, inputs, no_grad=True)
        assert off["trunk"].abs().max().item() > 0
        for k in ("trunk", "policy_logits", "baseline"):
            assert torch.equal(on[k], off[k]), k


# --------------------------------------------------------------------- route

FUSED_FWD = CONV1 + ["actor_section_nhwc", PLAIN(32), "actor_section_nhwc", PLAIN(32),
                     "actor_section_nhwc"]


@gpu
@requires_gpu
class TestRoute:
    @pytest.mark.parametrize("mode", ["a", "b"])
    def test_flag_takes_three_launches(self, mode, monkeypatch, default_switches):
        model = flagged(build_model({}, mode))
        rec = Recorder(monkeypatch)
        fwd, bwd = run(rec, model, mode == "b", True, monkeypatch, {})
        assert fwd == FUSED_FWD, fwd
        assert bwd == []

    @pytest.mark.parametrize("mode", ["a", "b"])
    def test_switch_and_grad_keep_the_default_route(self, mode, monkeypatch, default_switches):
        model = flagged(build_model({}, mode))
        rec = Recorder(monkeypatch)
        monkeypatch.setenv("MOOLIB_AMD_NO_ACTOR_SECTION", "1")
        fwd, _ = run(rec, model, mode == "b", True, monkeypatch, {})
        assert fwd == expected("default", True)[0], fwd
        monkeypatch.delenv("MOOLIB_AMD_NO_ACTOR_SECTION")
        fwd, bwd = run(rec, model, mode == "b", False, monkeypatch, {})
        assert (fwd, bwd) == expected("default", False), (fwd, bwd)


def test_flag_changes_nothing_on_cpu():
    from moolib_amd.models.atari import AtariNet

    torch.manual_seed(0)
    model = AtariNet(num_actions=6)
    g = torch.Generator().manual_seed(1)
    inputs = {"state": torch.randint(0, 256, (1, 2, 4, 84, 84), dtype=torch.uint8, generator=g),
              "reward": torch.zeros(1, 2), "done": torch.zeros(1, 2, dtype=torch.bool),
              "prev_action": torch.zeros(1, 2, dtype=torch.int64)}
    outs = []
    for on in (False, True):
        model.fused_actor_sections = on
        with torch.no_grad():
            outs.append(model(inputs, tuple())[0])
    for k in ("policy_logits", "baseline"):
        assert torch.equal(outs[0][k], outs[1][k]), k
    assert AtariNet(num_actions=6).fused_actor_sections is False
    assert AtariNet(num_actions=6, fused_actor_sections=True).fused_actor_sections is True


# ------------------------------------------------------------------- capture


@gpu
@requires_gpu
class TestCapture:
    def test_replay_reads_repacked_weights(self, default_switches):
        """The captured forward reads the persistent packs: after an in-place
        weight update and repack(), a replay gives the new weights' output."""
        from moolib_amd.ops import conv3x3 as c3
        from moolib_amd.parallel.graphs import GraphedCall

        params, frames, _ = int_case()
        model = flagged(build_model(params, "a"))
        inputs = {k: v.cuda() for k, v in int_inputs(frames[:2].transpose(0, 1).contiguous()).items()}
        assert inputs["state"].shape[:2] == (1, 2)

        def fwd(inp):
            with torch.no_grad():
                out = model(inp, tuple())[0]
            return {k: out[k] for k in ("policy_logits", "baseline")}

        call = GraphedCall(fwd, warmup=1, name="actor_section_test")
        call(inputs)
        old = {k: v.clone() for k, v in call(inputs).items()}
        assert call.graph is not None and not call.failed
        again = call(inputs)
        assert all(torch.equal(again[k], old[k]) for k in old)

        new_params, _, _ = int_case(TR.INT_SEED + 1)
        with torch.no_grad():
            for k, p in model.named_parameters():
                if k in new_params:
                    p.copy_(new_params[k])
        c3.repack(model)
        got = {k: v.clone() for k, v in call(inputs).items()}
        model.fused_actor_sections = False
        want = fwd(inputs)
        for k in got:
            assert torch.equal(got[k], want[k]), k
        assert not torch.equal(got["policy_logits"], old["policy_logits"])
