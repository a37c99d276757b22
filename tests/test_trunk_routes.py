"""Which entry points each route of the AtariNet trunk calls, in order.

tests/test_trunk_composed.py holds the trunk's values to a reference; it would
not notice a route that silently fell back to MIOpen, or a block that took
five launches where two were meant. Here every public callable of
`moolib_amd._kernels` and `torch.nn.functional.conv2d` is wrapped for one
forward (and backward), and the recorded sequence of names must equal the one
written down below from the route table in models/atari.py. A
`conv3x3_nhwc_fused` call is recorded with its fused prologue and epilogue.

Shapes: T=1, B=2, 84x84x4 frames (the 3872-wide fc fixes them), 6 actions, no
LSTM. Nothing past the trunk calls a recorded function.
"""
import contextlib

import pytest
import torch

from test_trunk_composed import BF16, build_model

gpu = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

SWITCHES = ("MOOLIB_AMD_CONV3_KERNEL", "MOOLIB_AMD_NO_FUSED_BIAS", "MOOLIB_AMD_NO_CONV1_KERNEL",
            "MOOLIB_AMD_NO_FRAMES_KERNEL", "MOOLIB_AMD_NO_POOL_KERNEL", "MOOLIB_AMD_WGRAD_KERNEL")
ENVS = {
    "default": {},
    "no_conv3": {"MOOLIB_AMD_CONV3_KERNEL": "0"},
    "no_fused_bias": {"MOOLIB_AMD_NO_FUSED_BIAS": "1"},
    "no_conv1": {"MOOLIB_AMD_NO_CONV1_KERNEL": "1"},
    "no_conv1_no_frames": {"MOOLIB_AMD_NO_CONV1_KERNEL": "1", "MOOLIB_AMD_NO_FRAMES_KERNEL": "1"},
    "no_pool": {"MOOLIB_AMD_NO_POOL_KERNEL": "1"},
}
CONV_ARGS = ("x", "w_packed", "k", "relu_in", "bias_in", "epi", "bias1", "res", "bias2", "rt")
CONV_DEFAULTS = {"relu_in": False, "bias_in": None, "epi": 0, "bias1": None, "res": None,
                 "bias2": None, "rt": 0}


# ------------------------------------------------------------------ recording


class Recorder:
    """Wraps the entry points on their module objects (the ops and nn.Conv2d
    look them up at call time) and lists the calls."""

    def __init__(self, monkeypatch):
        from moolib_amd import _kernels

        self.calls = []      # names; conv3x3_nhwc_fused as a tuple, see conv()
        self.packs = []      # w_packed.data_ptr() of every conv3x3_nhwc_fused call
        self.repacks = []    # argument lists of every repack3x3_batched call
        for name in dir(_kernels):
            fn = getattr(_kernels, name)
            if not name.startswith("_") and callable(fn):
                monkeypatch.setattr(_kernels, name, self._wrap(name, fn))
        monkeypatch.setattr(torch.nn.functional, "conv2d",
                            self._wrap("conv2d", torch.nn.functional.conv2d))

    def _wrap(self, name, fn):
        def wrapper(*args, **kwargs):
            out = fn(*args, **kwargs)
            if name == "conv3x3_nhwc_fused":
                a = dict(CONV_DEFAULTS, **dict(zip(CONV_ARGS, args)), **kwargs)
                self.calls.append(conv(a["relu_in"], a["bias_in"] is not None, a["epi"],
                                       a["bias2"] is not None, out.shape[1]))
                self.packs.append(a["w_packed"].data_ptr())
            else:
                self.calls.append(name)
            if name == "repack3x3_batched":
                self.repacks.append(args)
            return out

        return wrapper

    def take(self):
        calls, self.calls = self.calls, []
        return calls


def conv(relu_in, bias_in, epi, bias2, channels):
    """One conv3x3_nhwc_fused launch: relu on load, a bias added before that
    relu, the epilogue (0 none, 1 bias, 3 bias + residual), a second bias in
    the epilogue, output channels."""
    return ("conv3x3_nhwc_fused", relu_in, bias_in, epi, bias2, channels)


def run(rec, model, autocast, no_grad, monkeypatch, env):
    """(forward calls, backward calls) of one pass; the backward starts from
    the trunk output, which is what `model.fc` is handed."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g = torch.Generator().manual_seed(0)
    inputs = {"state": torch.randint(0, 256, (1, 2, 4, 84, 84), dtype=torch.uint8, generator=g).cuda(),
              "reward": torch.zeros(1, 2).cuda(), "done": torch.zeros(1, 2, dtype=torch.bool).cuda(),
              "prev_action": torch.zeros(1, 2, dtype=torch.int64).cuda()}
    seen = []
    handle = model.fc.register_forward_pre_hook(lambda m, args: seen.append(args[0]))
    amp = torch.autocast("cuda", dtype=BF16) if autocast else contextlib.nullcontext()
    rec.take()
    try:
        with amp, (torch.no_grad() if no_grad else contextlib.nullcontext()):
            model(inputs, tuple())
    finally:
        handle.remove()
    fwd = rec.take()
    (trunk,) = seen
    assert trunk.shape == (2, 3872)
    if not no_grad:
        trunk.backward(torch.randn(trunk.shape, generator=g).to(trunk.dtype).cuda())
        torch.cuda.synchronize()
    return fwd, rec.take()


# --------------------------------------------------------- expected sequences
#
# Written from the route table (models/atari.py). `cv` is what a bias-free
# conv records: PLAIN(channels) on the MFMA kernel, "conv2d" through MIOpen.


def PLAIN(channels):
    return conv(False, False, 0, False, channels)


def block_two_launches(ch, pending):
    """A block without grad on the MFMA kernel."""
    return [conv(True, pending, 0, False, ch), conv(True, True, 3, pending, ch)]


def block_fwd(cv, pending):
    """A block through forward_fused otherwise; the leading relu is F.relu
    unless a pending bias makes it bias_relu."""
    return (["bias_relu_fwd"] if pending else []) + [cv, "bias_relu_fwd", cv, "bias_add2_fwd"]


def block_bwd(dgrad, pending):
    """Backward of block_fwd: bias_add2's channel sum, conv1's dgrad (the
    weight gradient is MIOpen's, not recorded), bias_relu, conv0's dgrad, the
    leading bias_relu. `dgrad` is [] where the convs ran through MIOpen."""
    return (["channel_sum_fp32"] + dgrad + ["bias_relu_bwd"] + dgrad
            + (["bias_relu_bwd"] if pending else []))


POOL_F, POOL_B = ["maxpool3x3s2_fwd"], ["maxpool3x3s2_bwd"]
CONV1 = ["frames_u8_to_bf16_nhwc", conv(False, False, 1, False, 16)]
CONV1_BWD = ["wgrad3x3_nhwc", "channel_sum_fp32"]


def expected(env, no_grad):
    """(forward, backward) of the bf16 modes (a) and (b), which take the same
    routes."""
    mfma = env != "no_conv3"
    pf, pb = ([], []) if env == "no_pool" else (POOL_F, POOL_B)
    cv = {16: PLAIN(16) if mfma else "conv2d", 32: PLAIN(32) if mfma else "conv2d"}
    dg = {16: [PLAIN(16)] if mfma else [], 32: [PLAIN(32)] if mfma else []}

    if env == "no_fused_bias":
        # plain sections: nn.Conv2d with its bias, pool, blocks as modules
        fwd = CONV1 + pf + ["conv2d"] * 4 + (["conv2d"] + pf + ["conv2d"] * 4) * 2
        return (fwd, []) if no_grad else (fwd, pb * 3 + CONV1_BWD)

    def blocks(ch, pending):
        if no_grad and mfma:
            return block_two_launches(ch, pending) + block_two_launches(ch, False)
        return block_fwd(cv[ch], pending) + block_fwd(cv[ch], False)

    def blocks_bwd(ch, pending):
        return block_bwd(dg[ch], False) + block_bwd(dg[ch], pending)

    if env in ("no_conv1", "no_conv1_no_frames"):
        # section 0 as any other; its 4-channel conv is not an MFMA shape
        decode = ["frames_u8_to_bf16_nhwc"] if env == "no_conv1" else []
        fwd0 = decode + ["conv2d"] + pf + blocks(16, True)
        bwd0 = blocks_bwd(16, True) + pb
    else:
        fwd0 = CONV1 + pf + blocks(16, False)
        bwd0 = blocks_bwd(16, False) + pb + CONV1_BWD
    fwd = fwd0 + ([cv[32]] + pf + blocks(32, True)) * 2
    # the section conv's dgrad gives its input's channels: 32 into section 2, 16 into 1
    bwd = blocks_bwd(32, True) + pb + dg[32] + blocks_bwd(32, True) + pb + dg[16] + bwd0
    return (fwd, []) if no_grad else (fwd, bwd)


def expected_fp32():
    """fp32 weights, no autocast, under grad: eager stem, no MFMA conv, the
    fused bias ops and the pool kernel in fp32."""
    sec = ["conv2d"] + POOL_F + block_fwd("conv2d", True) + block_fwd("conv2d", False)
    sec_bwd = block_bwd([], False) + block_bwd([], True) + POOL_B
    return sec * 3, sec_bwd * 3


# ---------------------------------------------------------------------- tests


def test_expected_sequences_are_what_the_table_says():
    """The launch counts the project quotes, from the expectations alone."""
    fwd, bwd = expected("default", True)
    assert bwd == [] and len(fwd) == 1 + 15 + 3            # frames, 15 convs, 3 pools
    assert fwd.count(conv(True, True, 3, True, 32)) == 2   # the pending bias closes res0 twice
    fwd, bwd = expected("default", False)
    assert sum(c == PLAIN(16) or c == PLAIN(32) for c in fwd) == 14
    assert sum(c == PLAIN(16) or c == PLAIN(32) for c in bwd) == 14   # dgrad on the same kernel
    assert bwd[-2:] == CONV1_BWD
    fwd, _ = expected("no_conv3", True)
    assert fwd.count("conv2d") == 14 and fwd[:2] == CONV1  # conv1 does not ask available()
    fwd, _ = expected("no_fused_bias", True)
    assert fwd.count("conv2d") == 14 and "bias_relu_fwd" not in fwd


@gpu
@requires_gpu
class TestTrunkRoutes:
    @pytest.mark.parametrize("env", list(ENVS))
    @pytest.mark.parametrize("no_grad", [True, False], ids=["no_grad", "grad"])
    @pytest.mark.parametrize("mode", ["a", "b"])
    def test_bf16_routes(self, mode, no_grad, env, monkeypatch):
        model = build_model({}, mode)
        rec = Recorder(monkeypatch)
        fwd, bwd = run(rec, model, mode == "b", no_grad, monkeypatch, ENVS[env])
        want_fwd, want_bwd = expected(env, no_grad)
        assert fwd == want_fwd, ("forward", fwd)
        assert bwd == want_bwd, ("backward", bwd)

    def test_fp32_route(self, monkeypatch):
        from moolib_amd.models.atari import AtariNet

        torch.manual_seed(0)
        model = AtariNet(num_actions=6).cuda().to(memory_format=torch.channels_last)
        rec = Recorder(monkeypatch)
        fwd, bwd = run(rec, model, False, False, monkeypatch, {})
        want_fwd, want_bwd = expected_fp32()
        assert fwd == want_fwd, ("forward", fwd)
        assert bwd == want_bwd, ("backward", bwd)

    def test_repack_keeps_route_and_buffers(self, monkeypatch):
        """A second no-grad forward after repack(): one batched launch over
        the 15 packs the forward made (the first conv's padded to 8
        channels), the same sequence again, every pack at its address."""
        from moolib_amd.ops import conv3x3 as c3

        model = build_model({}, "a")
        rec = Recorder(monkeypatch)
        first, _ = run(rec, model, False, True, monkeypatch, {})
        packs, rec.packs = rec.packs, []
        assert first == expected("default", True)[0] and len(set(packs)) == 15
        c3.repack(model)
        assert rec.take() == ["repack3x3_batched"]
        (ws, fs, ds, cps), = rec.repacks
        convs = [m for m in model.modules() if isinstance(m, torch.nn.Conv2d)]
        assert [w.data_ptr() for w in ws] == [m.weight.data_ptr() for m in convs]
        assert [f.data_ptr() for f in fs] == packs          # forward order is module order
        assert all(d.numel() == 0 for d in ds)              # no backward ran: no dgrad pack
        assert list(cps) == [8] + [0] * 14
        second, _ = run(rec, model, False, True, monkeypatch, {})
        assert second == first
        assert rec.packs == packs
