"""The composed AtariNet (autograd Functions of ops/ and the wiring in
models/atari.py) against the fp64 reference in tests/trunk_refs.py.

docs/KERNEL_TESTS.md, "Composed trunk", has the arguments, the rounding
points and the recorded figures. Two kinds of GPU test, as for the kernels:

* integer-exact: the whole conv trunk through the real `AtariNet.forward` on
  inputs for which every value and every fp32 sum is a small integer, so the
  trunk output and every section parameter's gradient must be `torch.equal`
  to the reference;
* float: the whole network, every output and every parameter's gradient within
  `2 d + 2^-8 max|R_exact|` of R_exact, `d = max|R_emul - R_exact|` from the
  CPU alone.

The CPU part checks the reference against torch, asserts the premise of the
integer case, prints `d`, and shows that the comparisons reject six wiring
mistakes.
"""
import contextlib
import json

import pytest
import torch
import torch.nn.functional as F

import kernel_refs as R
import trunk_refs as TR

gpu = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

BF16 = torch.bfloat16
GRAD_DTYPE = {"a": torch.bfloat16, "b": torch.float32}
CONV_WEIGHTS = tuple(k for k in TR.SECTION_PARAMS if k.endswith("weight"))
# the first conv's weight gradient never goes through MIOpen
WRW_WEIGHTS = tuple(k for k in CONV_WEIGHTS if k != "sections.0.conv.weight")


def _figure(**kw):
    """One machine-readable line per measured figure (shown with pytest -s)."""
    print("KERNEL_EDGES_FIGURE " + json.dumps(kw))


# ---------------------------------------------------------- shared references

_cache = {}


def _once(key, fn):
    """References are computed once, shared between tests and never changed."""
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


# the integer case, and the one the weights are updated to in
# test_after_in_place_weight_update; TestIntegerPremise holds both to the premise
INT_SEEDS = (TR.INT_SEED, TR.INT_SEED + 1)


def int_case(seed=TR.INT_SEED):
    return _once(("int", seed), lambda: TR.integer_case(seed))


def int_ref(mode, wgrad, mutate=(), seed=TR.INT_SEED):
    """R_emul of the integer trunk case."""
    params, frames, G = int_case(seed)
    return _once(("int_emul", mode, wgrad, mutate, seed), lambda: TR.atari_ref(
        params, {"state": frames}, mode=mode, wgrad=wgrad, grads={"trunk": G}, mutate=mutate))


def int_exact(seed=TR.INT_SEED):
    params, frames, G = int_case(seed)
    return _once(("int_exact", seed),
                 lambda: TR.exact(params, {"state": frames}, grads={"trunk": G}))


def float_refs(use_lstm, mode, wgrad="wrw"):
    """(case, R_exact, R_emul) of the whole-network float case."""
    case = _once(("float", use_lstm), lambda: TR.float_case(use_lstm))
    params, inputs, core, grads = case
    ex = _once(("float_exact", use_lstm), lambda: TR.exact(params, inputs, core, grads))
    em = _once(("float_emul", use_lstm, mode, wgrad), lambda: TR.atari_ref(
        params, inputs, core, mode, wgrad, grads))
    return case, ex, em


def float_tensors(out):
    """name -> tensor for everything the float test compares."""
    t = {k: out[k] for k in ("policy_logits", "baseline", "hT", "cT") if k in out}
    t.update({"grad " + k: v for k, v in out["grads"].items()})
    return t


# ---------------------------------------------------------------- comparisons


def int_failures(got, ref, mode, names):
    """Names in `names` (plus the trunk output) that are not bit-equal to the
    reference cast to the dtype the path returns."""
    bad = []
    if not TR.bit_equal(got["trunk"], ref["trunk"], BF16):
        bad.append("trunk")
    for k in names:
        if k not in got["grads"] or not TR.bit_equal(got["grads"][k], ref["grads"][k],
                                                     GRAD_DTYPE[mode]):
            bad.append(k)
    return bad


def float_failures(got, exact, emul, figure=None):
    """Tensors of `got` beyond 2 d + 2^-8 max|R_exact| of R_exact."""
    ex, em = float_tensors(exact), float_tensors(emul)
    bad = []
    for k in ex:
        d, bound = TR.float_bound(ex[k], em[k])
        if k not in got:
            bad.append((k, "missing"))
            continue
        same = got[k].shape == ex[k].shape
        err = (got[k].double() - ex[k]).abs().max().item() if same else None
        if figure is not None:  # vs_emul: how well the emulation predicts the GPU path
            vs_emul = (got[k].double() - em[k]).abs().max().item() if same else None
            _figure(tensor=k, max_exact=ex[k].abs().max().item(), d=d, err=err, bound=bound,
                    vs_emul=vs_emul, **figure)
        if not TR.float_within(got[k], ex[k], bound):
            bad.append((k, err, bound))
    return bad


# ======================================================================= CPU


def torch_atari_fp64(params, inputs, core, grads):
    """The project's own CPU path (plain torch ops, NCHW) in float64."""
    from moolib_amd.models.atari import AtariNet

    use_lstm = "core.weight_hh_l0" in params
    model = AtariNet(num_actions=params["policy.weight"].shape[0], use_lstm=use_lstm).double()
    model.load_state_dict({k: v.double() for k, v in params.items()})
    cs = tuple(c.double() for c in core) if use_lstm else tuple()
    out, cs = model(inputs, cs)
    ((out["policy_logits"] * grads["policy_logits"].double()).sum()
     + (out["baseline"] * grads["baseline"].double()).sum()).backward()
    res = {"policy_logits": out["policy_logits"].detach(), "baseline": out["baseline"].detach(),
           "grads": {k: p.grad for k, p in model.named_parameters()}}
    if use_lstm:
        res["hT"], res["cT"] = cs[0][0].detach(), cs[1][0].detach()
    return res


class TestReferences:
    @pytest.mark.parametrize("shape", [(2, 8, 5, 7), (1, 3, 11, 11), (2, 2, 6, 4), (1, 2, 1, 1),
                                       (1, 1, 21, 21)])
    def test_pool_has_the_kernel_reference_tie_rule(self, shape):
        """Five input values: ties are the rule. Output and gradient routing
        equal maxpool3x3s2_ref's."""
        g = torch.Generator().manual_seed(sum(shape))
        x = torch.randint(-2, 3, shape, generator=g).double()
        N, C, H, W = shape
        gout = R.int_tensor(g, (N, C, (H + 1) // 2, (W + 1) // 2), -3, 3)
        if H * W > 1:  # the share test_kernel_edges.py asks of its pool inputs
            assert R.maxpool_tie_fraction(x) >= 0.2
        want, gin = R.maxpool3x3s2_ref(x, gout)
        xr = x.clone().requires_grad_()
        y = TR.maxpool(xr)
        y.backward(gout)
        assert torch.equal(y.detach(), want)
        assert torch.equal(xr.grad, gin)

    def test_conv_section_matches_torch(self):
        """One section with a pending bias (conv -> pool -> 2 blocks) against
        F.conv2d / F.max_pool2d / F.relu in fp64, on tie-free data."""
        g = torch.Generator().manual_seed(5)
        rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
        names = [k for k in TR.SECTION_PARAMS if k.startswith("sections.1.")]
        p = {k: (rn(32, 16 if k == "sections.1.conv.weight" else 32, 3, 3) * 0.1
                 if k.endswith("weight") else rn(32)).requires_grad_() for k in names}
        x0 = rn(2, 16, 9, 7)
        gy = rn(2, 32, 5, 4)

        def mine(x):
            u = TR.maxpool(TR.conv(x, p["sections.1.conv.weight"], False))
            u = TR.residual_block(u, p, "sections.1.res0.", False, p["sections.1.conv.bias"])
            return TR.residual_block(u, p, "sections.1.res1.", False)

        def theirs(x):
            c = lambda n, t: F.conv2d(t, p[n + ".weight"], p[n + ".bias"], padding=1)
            u = F.max_pool2d(c("sections.1.conv", x), 3, stride=2, padding=1)
            for r in ("sections.1.res0", "sections.1.res1"):
                u = u + c(r + ".conv1", F.relu(c(r + ".conv0", F.relu(u))))
            return u

        res = []
        for f in (mine, theirs):
            x = x0.clone().requires_grad_()
            with TR.rounding(False, False):
                y = f(x)
            gr = torch.autograd.grad(y, [x] + [p[k] for k in names], gy)
            res.append([y.detach()] + list(gr))
        for a, b in zip(*res):
            assert (a - b).abs().max().item() <= 1e-12 * max(1.0, b.abs().max().item())

    @pytest.mark.parametrize("use_lstm", [False, True])
    def test_exact_reference_matches_project_cpu_path(self, use_lstm):
        """R_exact against AtariNet itself on the CPU in float64 (plain torch
        ops, NCHW, nn.LSTM stepped in Python): outputs, core state and every
        parameter's gradient. 1e-6: the CPU path scales the frames by the
        double 1/255, the GPU path and the reference by the fp32 one."""
        (params, inputs, core, grads), ex, _ = float_refs(use_lstm, "a")
        want = float_tensors(torch_atari_fp64(params, inputs, core, grads))
        got = float_tensors(ex)
        assert set(got) == set(want) and len(got["grad fc.weight"]) == 256
        for k in want:
            err = (got[k] - want[k]).abs().max().item()
            assert err <= 1e-6 * max(want[k].abs().max().item(), 1e-3), (k, err)

    def test_lstm_node_with_rounding_off_equals_plain_recurrence(self):
        d = R.lstm_inputs(torch.Generator().manual_seed(3), 3, 4)
        res = []
        for force in (True, False):
            leaves = [d[k].clone().requires_grad_() for k in ("X", "h0", "c0", "w")]
            with TR.rounding(False, False):
                H, hT, cT = TR.lstm(*leaves, d["nd"], force_emul=force)
            loss = (H * d["gH"]).sum() + (hT * d["ghT"]).sum() + (cT * d["gcT"]).sum()
            res.append([H.detach(), hT.detach(), cT.detach()]
                       + list(torch.autograd.grad(loss, leaves)))
        ex = R.lstm_exact(d)
        for a, b, k in zip(res[0], res[1], R.LSTM_TENSORS):
            assert (a - b).abs().max().item() < 1e-12, k
            assert (b - ex[k]).abs().max().item() < 1e-12, k

    def test_q_rounds_value_and_gradient_to_nearest_even(self):
        x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 257.0, -0.3],
                         dtype=torch.float64, requires_grad=True)
        y = TR.Q(x)
        assert y.tolist()[:3] == [1.0, 1.0 + 2.0 ** -6, 256.0]  # ties go to even
        y.backward(torch.tensor([259.0, 1.0, 0.1, 3.0], dtype=torch.float64))
        assert torch.equal(x.grad, R.bf16_round(torch.tensor([259.0, 1.0, 0.1, 3.0]).double()))
        assert x.grad[0].item() == 260.0
        with TR.rounding(False, False):
            assert TR.Q(x) is x


class TestIntegerPremise:
    """What makes `torch.equal` a fair demand on the trunk, from the reference
    alone (no GPU). Seed and tap counts are fixed in trunk_refs; this is what
    guards them."""

    @pytest.mark.parametrize("seed", INT_SEEDS)
    def test_premise(self, seed):
        params, frames, G = int_case(seed)
        inputs = {"state": frames}
        with TR.probing() as fig:
            on = TR.atari_ref(params, inputs, mode="a", wgrad="kernel", grads={"trunk": G})
        with TR.rounding(act=False, param=True):
            off = TR.atari_ref(params, inputs, mode="a", wgrad="kernel", grads={"trunk": G})
        _figure(kind="trunk_premise", seed=seed, **fig)
        # the activation and activation-gradient roundings do nothing here ...
        assert torch.equal(on["trunk"], off["trunk"])
        assert set(on["grads"]) == set(TR.SECTION_PARAMS) == set(off["grads"])
        for k in TR.SECTION_PARAMS:
            assert torch.equal(on["grads"][k], off["grads"][k]), k
        # ... because every such value is an integer that bf16 holds
        assert fig["nonint"] == 0
        assert fig["act_max"] <= 256 and fig["grad_max"] <= 256
        # every fp32 sum (conv, dgrad, wgrad, bias gradient) is exact in any order
        assert fig["sum_max"] < 2 ** 24 and fig["pgrad_max"] < 2 ** 24
        # frames decode to exactly 0 and 1
        assert set(TR.decode_frames(frames.flatten(0, 1)).unique().tolist()) == {0.0, 1.0}
        # the case says something: no dead conv, no (nearly) empty gradient
        assert fig["live_min"] > 1
        shares = {k: (v != 0).double().mean().item() for k, v in on["grads"].items()}
        _figure(kind="trunk_premise", seed=seed, min_nonzero_share=min(shares.values()),
                trunk_max=on["trunk"].max().item(),
                trunk_nonzero=(on["trunk"] != 0).double().mean().item())
        assert min(shares.values()) >= 0.25, shares
        assert (on["trunk"] != 0).double().mean().item() >= 0.25
        # the exact reference differs from R_emul only where a large dW is rounded
        ex = int_exact(seed)
        assert torch.equal(ex["trunk"], on["trunk"])
        for k in TR.SECTION_PARAMS:
            assert torch.equal(R.bf16_round(ex["grads"][k]), on["grads"][k]), k
        # mode (b), project wgrad kernel: fp32 gradients, nothing is rounded
        b = int_ref("b", "kernel", seed=seed)
        for k in TR.SECTION_PARAMS:
            want = ex["grads"][k]
            if k.endswith("bias") and k != "sections.0.conv.bias":
                continue  # contributions are rounded to bf16 one by one
            assert torch.equal(b["grads"][k], want), k


FLOAT_CASES = [(False, "a"), (False, "b"), (True, "a"), (True, "b")]


class TestFloatDistance:
    @pytest.mark.parametrize("use_lstm,mode", FLOAT_CASES)
    def test_rounding_distance(self, use_lstm, mode):
        """d = max|R_emul - R_exact| per tensor, printed for the doc. Every
        tensor is there, none is identically zero, and R_emul is a
        perturbation of R_exact (d below the tensor's own magnitude; bf16
        rounding flips ReLU and pool selections, so single gradient elements
        move by far more than 2^-8 of the maximum)."""
        _, ex, em = float_refs(use_lstm, mode)
        ex, em = float_tensors(ex), float_tensors(em)
        assert set(ex) == set(em) and len(ex) == (2 + 36 if not use_lstm else 4 + 40)
        for k in ex:
            d, bound = TR.float_bound(ex[k], em[k])
            scale = ex[k].abs().max().item()
            _figure(kind="trunk_float_d", lstm=use_lstm, mode=mode, tensor=k, max_exact=scale,
                    d=d, bound=bound)
            assert scale > 0, k
            assert d <= scale, (k, d, scale)


def _mutants():
    """name -> (mutate flags of the reference, edit of its output, tensor that
    must be rejected)."""
    pend = "grad sections.1.conv.bias"

    def double(out):
        out["grads"]["sections.2.res0.conv1.bias"] = out["grads"]["sections.2.res0.conv1.bias"] * 2

    def swap(out):
        k = "sections.1.res1.conv0.weight"
        out["grads"][k] = out["grads"][k].transpose(2, 3).contiguous()

    def padded(out):
        k = "sections.0.conv.weight"  # channels 4..7 of the padded input are zero
        out["grads"][k] = torch.zeros_like(out["grads"][k])

    return {
        "pending_bias_grad_without_bias_add2": (("no_b2_grad",), None, pend),
        "bias_grad_doubled": ((), double, "grad sections.2.res0.conv1.bias"),
        "dw_kh_kw_swapped": ((), swap, "grad sections.1.res1.conv0.weight"),
        "conv1_dw_from_padded_channels": ((), padded, "grad sections.0.conv.weight"),
        "residual_add_drops_bias2": (("drop_bias2",), None, "trunk"),
        "trunk_flattened_nhwc": (("flatten_nhwc",), None, "trunk"),
    }


class TestComparisonsCanFail:
    """Each wiring mistake, applied to the reference (or to a copy of its
    output), is rejected by the comparison the GPU tests use; the unmutated
    reference passes it."""

    @staticmethod
    def _as_gpu(out, mode):
        """A reference output in the dtypes the GPU path returns."""
        res = {"trunk": out["trunk"].to(BF16),
               "grads": {k: v.to(GRAD_DTYPE[mode]) for k, v in out["grads"].items()}}
        return res

    @pytest.mark.parametrize("mode", ["a", "b"])
    def test_unmutated_reference_passes(self, mode):
        ref = int_ref(mode, "kernel")
        assert int_failures(self._as_gpu(ref, mode), ref, mode, TR.SECTION_PARAMS) == []
        for use_lstm in (False, True):
            _, ex, em = float_refs(use_lstm, mode)
            assert float_failures(float_tensors(em), ex, em) == []

    @pytest.mark.parametrize("name", list(_mutants()))
    @pytest.mark.parametrize("mode", ["a", "b"])
    def test_integer_comparison_rejects(self, name, mode):
        flags, edit, target = _mutants()[name]
        ref = int_ref(mode, "kernel")
        mut = int_ref(mode, "kernel", flags) if flags else ref
        mut = {"trunk": mut["trunk"], "grads": dict(mut["grads"])}
        if edit is not None:
            edit(mut)
        bad = int_failures(self._as_gpu(mut, mode), ref, mode, TR.SECTION_PARAMS)
        assert target.replace("grad ", "") in bad, bad

    def test_wrw_comparison_rejects(self):
        """The per-element bound of the MIOpen leg: one bf16 rounding of the
        exact value passes, two steps off or a swapped kernel do not."""
        k = "sections.1.res1.conv0.weight"
        want = int_exact()["grads"][k]
        assert TR.wrw_within(want.to(BF16), want)
        assert TR.wrw_within(want.float(), want)
        assert not TR.wrw_within((want * (1 + 2.0 ** -7)).to(BF16), want)
        assert not TR.wrw_within(want.transpose(2, 3).to(BF16), want)
        assert not TR.wrw_within((want * 2).to(BF16), want)
        assert not TR.wrw_within(torch.zeros_like(want).to(BF16), want)

    @pytest.mark.parametrize("name", list(_mutants()))
    def test_float_comparison_rejects(self, name):
        flags, edit, target = _mutants()[name]
        (params, inputs, core, grads), ex, em = float_refs(False, "a")
        mut = em
        if flags:
            mut = _once(("float_mut", flags), lambda: TR.atari_ref(
                params, inputs, core, "a", "wrw", grads, flags))
        mut = dict(mut, grads=dict(mut["grads"]))
        if edit is not None:
            edit(mut)
        bad = [b[0] for b in float_failures(float_tensors(mut), ex, em)]
        if target == "trunk":  # the float test sees the trunk through the outputs
            assert "policy_logits" in bad and "baseline" in bad, bad
        else:
            assert target in bad, bad


# ======================================================================= GPU


def build_model(params, mode, use_lstm=False, num_actions=6):
    """AtariNet on the GPU holding `params`: (a) bf16 shadow weights,
    channels_last, as ImpalaPeer builds fwd_model; (b) fp32 master weights
    (run under autocast), as R2D2Learner holds its online network."""
    from moolib_amd.models.atari import AtariNet

    torch.manual_seed(0)
    model = AtariNet(num_actions=num_actions, use_lstm=use_lstm)
    sd = model.state_dict()
    sd.update({k: v.float() for k, v in params.items()})
    model.load_state_dict(sd)
    model = model.cuda()
    if mode == "a":
        model = model.to(BF16).to(memory_format=torch.channels_last)
    return model


def run_model(model, mode, inputs, core=None, grads=None, no_grad=False):
    """One forward (and backward) through the real AtariNet.forward. The trunk
    output is what `model.fc` is handed; {"trunk": G} backpropagates G from
    there."""
    seen = []
    handle = model.fc.register_forward_pre_hook(lambda m, args: seen.append(args[0]))
    inputs = {k: v.cuda() for k, v in inputs.items()}
    core = tuple(c.cuda() for c in core) if core is not None else tuple()
    amp = torch.autocast("cuda", dtype=BF16) if mode == "b" else contextlib.nullcontext()
    try:
        with amp, (torch.no_grad() if no_grad else contextlib.nullcontext()):
            out, core_out = model(inputs, core)
    finally:
        handle.remove()
    (trunk,) = seen
    if grads is not None and "trunk" in grads:
        trunk.backward(grads["trunk"].to(trunk.dtype).cuda())
    elif grads is not None:
        ((out["policy_logits"] * grads["policy_logits"].cuda()).sum()
         + (out["baseline"] * grads["baseline"].cuda()).sum()).backward()
    res = {"trunk": trunk.detach().cpu(),
           "policy_logits": out["policy_logits"].detach().cpu(),
           "baseline": out["baseline"].detach().cpu(),
           "grads": {k: p.grad.cpu() for k, p in model.named_parameters() if p.grad is not None}}
    if core_out:
        res["hT"], res["cT"] = core_out[0][0].detach().cpu(), core_out[1][0].detach().cpu()
    return res


def int_inputs(frames):
    T, B = frames.shape[:2]
    return {"state": frames, "reward": torch.zeros(T, B), "done": torch.zeros(T, B, dtype=torch.bool),
            "prev_action": torch.zeros(T, B, dtype=torch.int64)}


@gpu
@requires_gpu
class TestTrunkIntegerExact:
    @pytest.mark.parametrize("wgrad", ["kernel", "wrw"])
    @pytest.mark.parametrize("mode", ["a", "b"])
    def test_forward_and_every_section_gradient(self, mode, wgrad, monkeypatch):
        """Trunk output, all section bias gradients and the first conv's weight
        gradient bit-equal in every leg; all conv weight gradients bit-equal
        under the project's wgrad kernel; under MIOpen's wrw within one bf16
        rounding of the exact value per element."""
        if wgrad == "kernel":
            monkeypatch.setenv("MOOLIB_AMD_WGRAD_KERNEL", "1")
        else:
            monkeypatch.delenv("MOOLIB_AMD_WGRAD_KERNEL", raising=False)
        params, frames, G = int_case()
        ref = int_ref(mode, wgrad)
        model = build_model(params, mode)
        assert all(p.grad is None for p in model.parameters())
        got = run_model(model, mode, int_inputs(frames), grads={"trunk": G})
        assert set(TR.SECTION_PARAMS) <= set(got["grads"])
        strict = [k for k in TR.SECTION_PARAMS if wgrad == "kernel" or k not in WRW_WEIGHTS]
        assert len(strict) == (30 if wgrad == "kernel" else 16)
        bad = int_failures(got, ref, mode, strict)
        if wgrad == "wrw":
            ex = int_exact()
            equal = [k for k in WRW_WEIGHTS
                     if TR.bit_equal(got["grads"][k], ref["grads"][k], GRAD_DTYPE[mode])]
            _figure(kind="trunk_int_wrw", mode=mode, bit_equal=len(equal), of=len(WRW_WEIGHTS),
                    not_equal=sorted(set(WRW_WEIGHTS) - set(equal)))
            bad += [k for k in WRW_WEIGHTS
                    if got["grads"][k].dtype != GRAD_DTYPE[mode]
                    or not TR.wrw_within(got["grads"][k], ex["grads"][k])]
        assert not bad, bad

    @pytest.mark.parametrize("mode", ["a", "b"])
    def test_no_grad_path(self, mode):
        """(c): the actor / R2D2-target path, two fused launches per block,
        must give the autograd path's trunk output bit for bit."""
        params, frames, _ = int_case()
        got = run_model(build_model(params, mode), mode, int_inputs(frames), no_grad=True)
        assert TR.bit_equal(got["trunk"], int_ref(mode, "kernel")["trunk"], BF16)
        assert torch.equal(int_ref("a", "kernel")["trunk"], int_ref("b", "wrw")["trunk"])


    @pytest.mark.parametrize("mode", ["a", "b"])
    def test_after_in_place_weight_update(self, mode, monkeypatch):
        """The convs read packed copies of the weights (forward, dgrad and the
        first conv's 8-channel pack), cached per module. After an in-place
        update, as an optimizer step makes it, every path must see the new
        weights: (a) through `repack()`, which ImpalaPeer calls after each
        step; (b) through the caches' version check alone, on which
        R2D2Learner relies."""
        from moolib_amd.ops import conv3x3 as c3

        monkeypatch.setenv("MOOLIB_AMD_WGRAD_KERNEL", "1")
        params, frames, G = int_case(INT_SEEDS[0])
        model = build_model(params, mode)
        run_model(model, mode, int_inputs(frames), grads={"trunk": G})
        run_model(model, mode, int_inputs(frames), no_grad=True)
        assert "c8" in model.sections[0].conv._c3_packs
        for conv in (model.sections[1].conv, model.sections[2].res1.conv1):
            assert "fwd" in conv._c3_packs and "dgrad" in conv._c3_packs
        params, frames, G = int_case(INT_SEEDS[1])
        with torch.no_grad():
            for k, p in model.named_parameters():
                if k in params:
                    p.copy_(params[k])
        model.zero_grad(set_to_none=True)
        if mode == "a":
            c3.repack(model)
        ref = int_ref(mode, "kernel", seed=INT_SEEDS[1])
        assert not torch.equal(ref["trunk"], int_ref(mode, "kernel")["trunk"])
        got = run_model(model, mode, int_inputs(frames), grads={"trunk": G})
        assert int_failures(got, ref, mode, TR.SECTION_PARAMS) == []
        got = run_model(model, mode, int_inputs(frames), no_grad=True)
        assert TR.bit_equal(got["trunk"], ref["trunk"], BF16)


@gpu
@requires_gpu
class TestNetworkFloat:
    @pytest.mark.parametrize("use_lstm,mode", FLOAT_CASES)
    def test_outputs_and_every_gradient(self, use_lstm, mode, monkeypatch):
        """Whole network, default (MIOpen wrw) weight gradients: per tensor
        max|kernel - R_exact| <= 2 d + 2^-8 max|R_exact|."""
        monkeypatch.delenv("MOOLIB_AMD_WGRAD_KERNEL", raising=False)
        (params, inputs, core, grads), ex, em = float_refs(use_lstm, mode)
        model = build_model(params, mode, use_lstm)
        got = run_model(model, mode, inputs, core, grads)
        assert set(got["grads"]) == set(params)
        for k, v in got["grads"].items():
            assert v.dtype == GRAD_DTYPE[mode], k
        bad = float_failures(float_tensors(got), ex, em,
                             figure={"kind": "trunk_float", "lstm": use_lstm, "mode": mode})
        assert not bad, bad
