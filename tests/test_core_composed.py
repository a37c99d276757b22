"""The LSTM core of AtariNet as models/atari.py wires it, at every width that
has a fused scan (128, 256, 512) and on every opt-in route (`fused_trunk_fc`,
`fused_core_input`, `fused_core_recurrent`, `fused_actor_sections`), against
the fp64 reference in tests/trunk_refs.py.

docs/KERNEL_TESTS.md, "Composed core", has the rounding points per route, the
case and the recorded figures. The kernels' tile and slab edges are held by
the kernel-level tests; what is held here is the wiring, on one small case
(`trunk_refs.core_float_case`: T=3, B=3, a non-zero initial state, a row that
is done at t=0, rewards on both sides of the clamp):

* float: every output, the returned core state, the gradient of every
  parameter and of the initial state within `2 d + 2^-8 max|R_exact|` of
  R_exact, `d = max|R_emul - R_exact|` from the CPU alone;
* exact relations between routes that the route table promises;
* the actor's use of the core: T=1 calls that carry the state.

The CPU part checks the extended reference against the project's own CPU
code, asserts the premise of the case, and shows that the float comparison
rejects nine wiring mistakes.
"""
import contextlib
import json
import time

import pytest
import torch

import kernel_refs as R
import trunk_refs as TR

gpu = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

BF16 = torch.bfloat16
GRAD_DTYPE = {"a": torch.bfloat16, "b": torch.float32}
WIDTHS = (128, 256, 512)
OFF = ()
ALL_ON = ("trunk_fc", "core_input", "core_recurrent")
OUTPUTS = ("policy_logits", "baseline", "hT", "cT")
A = 6


def _figure(**kw):
    """One machine-readable line per measured figure (shown with pytest -s)."""
    print("KERNEL_EDGES_FIGURE " + json.dumps(kw))


# ---------------------------------------------------------- shared references

_cache = {}
_cpu_seconds = [0.0]


def _once(key, fn):
    """References are computed once, shared between tests and never changed."""
    if key not in _cache:
        t0 = time.perf_counter()
        _cache[key] = fn()
        _cpu_seconds[0] += time.perf_counter() - t0
    return _cache[key]


def case(lstm_size):
    return _once(("case", lstm_size), lambda: TR.core_float_case(lstm_size, A=A))


def _trunk(kind):
    """The trunk's forward with its graph: frames and section parameters are
    the same for every width, so one per kind ("exact", "a", "b") serves all."""
    params, inputs, _, _ = case(WIDTHS[0])
    frames = inputs["state"].flatten(0, 1)

    def build():
        if kind == "exact":
            with TR.rounding(False, False):
                return TR.trunk_graph(params, frames, "a", "kernel")
        return TR.trunk_graph(params, frames, kind, "wrw")

    return _once(("trunk", kind), build)


def exact_ref(lstm_size):
    params, inputs, core, grads = case(lstm_size)
    return _once(("exact", lstm_size), lambda: TR.exact(
        params, inputs, core, grads, trunk_cache=_trunk("exact")))


def emul_ref(lstm_size, mode, routes=OFF, mutate=()):
    """R_emul of the default (MIOpen) weight-gradient leg on `routes`."""
    params, inputs, core, grads = case(lstm_size)
    return _once(("emul", lstm_size, mode, tuple(sorted(routes)), mutate), lambda: TR.atari_ref(
        params, inputs, core, mode, "wrw", grads, mutate, trunk_cache=_trunk(mode),
        **{r: True for r in routes}))


def float_tensors(out):
    """name -> tensor for everything the float test compares."""
    t = {k: out[k] for k in OUTPUTS + ("dh0", "dc0") if k in out}
    t.update({"grad " + k: v for k, v in out["grads"].items()})
    return t


def float_failures(got, exact, emul, figure=None, only=None):
    """Tensors of `got` beyond 2 d + 2^-8 max|R_exact| of R_exact."""
    ex, em = float_tensors(exact), float_tensors(emul)
    bad = []
    for k in ex:
        if only is not None and k not in only:
            continue
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


def torch_atari_fp64(lstm_size, routes=OFF):
    """The project's own CPU path (plain torch ops, nn.LSTM stepped in Python)
    in float64 on the core case."""
    from moolib_amd.models.atari import AtariNet

    params, inputs, core, grads = case(lstm_size)
    model = AtariNet(num_actions=A, use_lstm=True, lstm_size=lstm_size,
                     **{"fused_" + r: True for r in routes}).double()
    model.load_state_dict({k: v.double() for k, v in params.items()})
    cs = tuple(c.double().requires_grad_() for c in core)
    out, cs_out = model(inputs, cs)
    ((out["policy_logits"] * grads["policy_logits"].double()).sum()
     + (out["baseline"] * grads["baseline"].double()).sum()
     + (cs_out[0][0] * grads["hT"].double()).sum()
     + (cs_out[1][0] * grads["cT"].double()).sum()).backward()
    return {"policy_logits": out["policy_logits"].detach(), "baseline": out["baseline"].detach(),
            "hT": cs_out[0][0].detach(), "cT": cs_out[1][0].detach(),
            "dh0": cs[0].grad[0], "dc0": cs[1].grad[0],
            "grads": {k: p.grad for k, p in model.named_parameters()}}


def _assert_close(got, want, tol=1e-6):
    got, want = float_tensors(got), float_tensors(want)
    assert set(got) == set(want) and len(got) == 6 + 40
    for k in want:
        err = (got[k] - want[k]).abs().max().item()
        assert err <= tol * max(want[k].abs().max().item(), 1e-3), (k, err)


class TestCoreReference:
    @pytest.mark.parametrize("lstm_size", [128, 512])
    def test_exact_reference_matches_project_cpu_path(self, lstm_size):
        """R_exact against AtariNet(lstm_size) on the CPU in float64: outputs,
        returned state, every parameter's gradient, dh0 and dc0 (1e-6: the CPU
        path scales the frames by the double 1/255)."""
        ex = exact_ref(lstm_size)
        assert ex["hT"].shape == (3, lstm_size)
        _assert_close(ex, _once(("torch", lstm_size), lambda: torch_atari_fp64(lstm_size)))

    @pytest.mark.parametrize("route", ALL_ON)
    def test_exact_reference_does_not_depend_on_the_route(self, route):
        """With every Q off each route's formula is the default one (1e-12),
        and AtariNet on the CPU with the flag set, where the flag's eager code
        runs or the flag does nothing, still agrees with it (1e-6)."""
        params, inputs, core, grads = case(128)
        with_flag = TR.exact(params, inputs, core, grads, trunk_cache=_trunk("exact"),
                             **{route: True})
        _assert_close(with_flag, exact_ref(128), 1e-12)
        _assert_close(with_flag, torch_atari_fp64(128, (route,)))

    def test_route_formulas_match_the_eager_ops(self):
        """On the CPU the model takes the per-step nn.LSTM loop, so its flags
        never reach `core_input_eager` / `trunk_fc_eager`; the reference's two
        route formulas are held to those functions directly, value and every
        gradient, in float64 with every Q off."""
        from moolib_amd.ops import fc as fc_ops
        from moolib_amd.ops import lstm as lstm_ops

        g = torch.Generator().manual_seed(11)
        rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
        M, Hd = 7, 8
        reward = torch.tensor([1.0, -1.0, 3.0, -2.5, 0.3337, 0.0, 0.9], dtype=torch.float64)
        action = torch.tensor([0, A - 1, 2, 2, 1, 0, A - 1])
        for fused in (False, True):
            res = []
            for fn in ("ref", "eager"):
                feat, w, bi, bh = (t.clone().requires_grad_() for t in (
                    rn(M, 256), rn(4 * Hd, 257 + A) * 0.1, rn(4 * Hd), rn(4 * Hd)))
                g.manual_seed(11)
                with TR.rounding(False, False):
                    y = (TR.core_input_proj(feat, reward, action, w, bi, bh, fused) if fn == "ref"
                         else lstm_ops.core_input_eager(feat, reward, action, w, bi, bh))
                gy = torch.linspace(-1, 1, y.numel(), dtype=torch.float64).view_as(y)
                res.append([y.detach()] + list(torch.autograd.grad(y, [feat, w, bi, bh], gy)))
            for a_, b_ in zip(*res):
                assert (a_ - b_).abs().max().item() <= 1e-12 * max(1.0, b_.abs().max().item())
        for fused in (False, True):
            res = []
            for fn in ("ref", "eager"):
                g.manual_seed(12)
                x, w, b = (t.clone().requires_grad_() for t in (
                    rn(3, 32, 2, 3), rn(256, 192) * 0.1, rn(256)))
                with TR.rounding(False, False):
                    y = (TR.fc_relu(torch.relu(x).reshape(3, -1), w, b, fused) if fn == "ref"
                         else fc_ops.trunk_fc_eager(x, w, b, relu_in=True))
                gy = torch.linspace(-1, 1, y.numel(), dtype=torch.float64).view_as(y)
                res.append([y.detach()] + list(torch.autograd.grad(y, [x, w, b], gy)))
            for a_, b_ in zip(*res):
                assert (a_ - b_).abs().max().item() <= 1e-12 * max(1.0, b_.abs().max().item())

    def test_routes_move_rounding_points_only_where_the_doc_says(self):
        """R_emul per route at 128: `core_recurrent` changes nothing at all;
        `trunk_fc` changes no forward value, and in (a) no gradient either."""
        for mode in ("a", "b"):
            base = float_tensors(emul_ref(128, mode))
            rec = float_tensors(emul_ref(128, mode, ("core_recurrent",)))
            assert all(torch.equal(base[k], rec[k]) for k in base)
        fc_a = float_tensors(emul_ref(128, "a", ("trunk_fc",)))
        base = float_tensors(emul_ref(128, "a"))
        assert all(torch.equal(base[k], fc_a[k]) for k in base)
        fc_b = float_tensors(emul_ref(128, "b", ("trunk_fc",)))
        base = float_tensors(emul_ref(128, "b"))
        differ = sorted(k for k in base if not torch.equal(base[k], fc_b[k]))
        assert differ == ["grad fc.bias", "grad fc.weight"], differ


class TestCasePremise:
    @pytest.mark.parametrize("lstm_size", WIDTHS)
    def test_premise(self, lstm_size):
        params, inputs, (h0, c0), grads = case(lstm_size)
        shared, inputs0, _, _ = case(WIDTHS[0])
        for k in TR.SECTION_PARAMS + ("fc.weight", "fc.bias"):
            assert torch.equal(params[k], shared[k]), k
        assert all(torch.equal(inputs[k], inputs0[k]) for k in inputs)
        assert all(torch.equal(v, R.bf16_round(v)) for v in params.values())
        assert params["core.weight_hh_l0"].shape == (4 * lstm_size, lstm_size)
        # the state: non-zero, h0 bf16-representable, c0 not
        assert h0.dtype == c0.dtype == torch.float32 and h0.shape == (1, 3, lstm_size)
        assert torch.equal(h0.double(), R.bf16_round(h0.double())) and h0.abs().max() > 0.5
        assert not torch.equal(c0.double(), R.bf16_round(c0.double()))
        # done: row 0 at t=0 only, row 1 at t=1, row 2 never
        assert inputs["done"].tolist() == [[True, False, False], [False, True, False],
                                           [False, False, False]]
        # reward: both clamp edges exactly, both sides beyond, one that bf16 does not hold
        r = inputs["reward"].flatten().double()
        assert (r == 1).any() and (r == -1).any() and (r > 1).any() and (r < -1).any()
        inside = r[(r > -1) & (r < 1)]
        assert (inside != R.bf16_round(inside)).any()
        assert inputs["reward"][0, 2].double() != R.bf16_round(inputs["reward"][0, 2].double())
        pa = inputs["prev_action"]
        assert (pa == 0).any() and (pa == A - 1).any() and pa.min() >= 0 and pa.max() < A
        # the probe unit: a rounding tie in c0, and a cT that cancels
        u = TR.CORE_PROBE_UNIT
        assert c0[0, 2, u].item() == TR.CORE_PROBE_C0
        assert R.bf16_round(c0[0, 2, u].double()).item() == 3.0
        ex = exact_ref(lstm_size)
        assert abs(ex["cT"][2, u].item()) < 0.1 and ex["cT"].abs().max().item() < 1.0
        # row 0 is done at t=0: no gradient reaches its initial state, the others' do
        assert not ex["dh0"][0].any() and not ex["dc0"][0].any()
        assert ex["dh0"][1].any() and ex["dh0"][2].any() and ex["dc0"][2].any()
        # every tensor is there and none is identically zero
        t = float_tensors(ex)
        assert len(t) == 6 + 40 and all(v.abs().max().item() > 0 for v in t.values())


# name -> the tensor that the mistake most directly affects
MUTANTS = {
    "reward_unclamped": "grad core.weight_ih_l0",
    "action_shifted": "grad core.weight_ih_l0",
    "no_bias_hh": "hT",
    "bias_hh_no_grad": "grad core.bias_hh_l0",
    "dw_hh_unshifted": "grad core.weight_hh_l0",
    "h0_unmasked": "dh0",
    "state_from_t_minus_2": "cT",
    "c0_bf16": "cT",
    "whh_i_f_swapped": "grad core.weight_hh_l0",
}


class TestCoreComparisonsCanFail:
    """Each wiring mistake, applied inside the reference, is rejected by the
    comparison the GPU tests use; the unmutated R_emul passes it."""

    @pytest.mark.parametrize("mode", ["a", "b"])
    @pytest.mark.parametrize("routes", [OFF, ALL_ON])
    def test_unmutated_reference_passes(self, mode, routes):
        em = emul_ref(128, mode, routes)
        assert float_failures(float_tensors(em), exact_ref(128), em) == []

    def test_every_mutation_is_listed(self):
        assert set(MUTANTS) == set(TR.CORE_MUTATIONS)

    @pytest.mark.parametrize("routes", [OFF, ALL_ON])
    @pytest.mark.parametrize("name", list(MUTANTS))
    def test_float_comparison_rejects(self, name, routes):
        mut = emul_ref(128, "a", routes, (name,))
        bad = [b[0] for b in float_failures(float_tensors(mut), exact_ref(128),
                                            emul_ref(128, "a", routes))]
        assert MUTANTS[name] in bad, bad


def test_cpu_seconds_of_the_reference_work():
    """Printed for the doc: what the references computed so far have cost."""
    _figure(kind="core_ref_cpu_seconds", seconds=round(_cpu_seconds[0], 1), entries=len(_cache))


# ======================================================================= GPU


def build_model(lstm_size, mode, routes=OFF, actor_sections=False):
    """AtariNet on the GPU holding the case's parameters: (a) bf16 shadow
    weights, channels_last, as ImpalaPeer builds fwd_model; (b) fp32 master
    weights (run under autocast), as R2D2Learner holds its online network."""
    from moolib_amd.models.atari import AtariNet

    params = case(lstm_size)[0]
    model = AtariNet(num_actions=A, use_lstm=True, lstm_size=lstm_size,
                     fused_actor_sections=actor_sections,
                     **{"fused_" + r: True for r in routes})
    model.load_state_dict({k: v.float() for k, v in params.items()})
    model = model.cuda()
    if mode == "a":
        model = model.to(BF16).to(memory_format=torch.channels_last)
    return model


def run_model(model, mode, inputs, core, grads=None, no_grad=False):
    """One forward (and backward) through the real AtariNet.forward; the core
    state goes in as fp32 leaves, as `initial_state()` gives it."""
    inputs = {k: v.cuda() for k, v in inputs.items()}
    core = tuple(c.cuda().requires_grad_(grads is not None) for c in core)
    amp = torch.autocast("cuda", dtype=BF16) if mode == "b" else contextlib.nullcontext()
    model.zero_grad(set_to_none=True)
    seen = []  # the tensor entering fc, kept for its gradient (default FC route only)

    def keep(module, args):
        seen.append(args[0])
        if args[0].requires_grad:
            args[0].retain_grad()

    handle = model.fc.register_forward_pre_hook(keep)
    try:
        with amp, (torch.no_grad() if no_grad else contextlib.nullcontext()):
            out, core_out = model(inputs, core)
    finally:
        handle.remove()
    assert core_out[0].dtype == core_out[1].dtype == torch.float32
    if grads is not None:
        ((out["policy_logits"] * grads["policy_logits"].cuda()).sum()
         + (out["baseline"] * grads["baseline"].cuda()).sum()
         + (core_out[0][0] * grads["hT"].cuda()).sum()
         + (core_out[1][0] * grads["cT"].cuda()).sum()).backward()
    res = {"policy_logits": out["policy_logits"].detach().cpu(),
           "baseline": out["baseline"].detach().cpu(),
           "hT": core_out[0][0].detach().cpu(), "cT": core_out[1][0].detach().cpu(),
           "grads": {k: p.grad.cpu() for k, p in model.named_parameters() if p.grad is not None}}
    if grads is not None:
        res["dh0"], res["dc0"] = core[0].grad[0].cpu(), core[1].grad[0].cpu()
        if seen:
            res["d_trunk"] = seen[0].grad.cpu()
    return res


@pytest.fixture
def calls(monkeypatch):
    """Counts of the entry points that tell the routes apart."""
    from moolib_amd import _kernels
    from moolib_amd.ops import conv3x3 as c3
    from moolib_amd.ops import fc as fc_ops
    from moolib_amd.ops import lstm as lstm_ops

    monkeypatch.delenv("MOOLIB_AMD_WGRAD_KERNEL", raising=False)
    seen = {}

    def wrap(mod, name, key=None):
        fn = getattr(mod, name)

        def counted(*a, **kw):
            k = key(a) if key else name
            seen[k] = seen.get(k, 0) + 1
            return fn(*a, **kw)

        monkeypatch.setattr(mod, name, counted)

    wrap(lstm_ops, "core_input_projection")
    wrap(fc_ops, "trunk_fc")
    wrap(c3, "actor_section")
    wrap(_kernels, "lstm_whh_pack")
    wrap(_kernels, "lstm_whh_grad")
    wrap(_kernels, "lstm_fused_fwd")
    wrap(_kernels, "lstm_wide_fwd", lambda a: "lstm_wide_fwd_saving" if a[5] else
         "lstm_wide_fwd_forward_only")
    return seen


def expected_calls(lstm_size, routes, no_grad=False, actor_sections=False, forwards=1):
    """What one forward (and backward, unless `no_grad`) must have called."""
    want = {}
    if "core_input" in routes:
        want["core_input_projection"] = forwards
    if "trunk_fc" in routes:
        want["trunk_fc"] = forwards
    if "core_recurrent" in routes:
        want["lstm_whh_pack"] = forwards
        if not no_grad:
            want["lstm_whh_grad"] = forwards
    if lstm_size == 256:
        want["lstm_fused_fwd"] = forwards
    else:
        want["lstm_wide_fwd_forward_only" if no_grad else "lstm_wide_fwd_saving"] = forwards
    if actor_sections:
        want["actor_section"] = 3 * forwards
    return want


FLOAT_CASES = [(w, r, m) for w in WIDTHS for r in (OFF, ALL_ON) for m in ("a", "b")]
FLOAT_CASES += [(512, (r,), "b") for r in ALL_ON]
_ids = lambda v: "+".join(v) or "off" if isinstance(v, tuple) else None


@gpu
@requires_gpu
class TestCoreFloat:
    @pytest.mark.parametrize("lstm_size,routes,mode", FLOAT_CASES, ids=_ids)
    def test_outputs_state_and_every_gradient(self, lstm_size, routes, mode, calls):
        """Per tensor max|kernel - R_exact| <= 2 d + 2^-8 max|R_exact|:
        outputs, returned state, 40 parameter gradients, dh0 and dc0; and the
        route under test is the one that ran."""
        _, inputs, core, grads = case(lstm_size)
        ex, em = exact_ref(lstm_size), emul_ref(lstm_size, mode, routes)
        model = build_model(lstm_size, mode, routes)
        got = run_model(model, mode, inputs, core, grads)
        assert calls == expected_calls(lstm_size, routes), calls
        assert set(got["grads"]) == set(ex["grads"]) and len(got["grads"]) == 40
        for k, v in got["grads"].items():
            assert v.dtype == GRAD_DTYPE[mode], k
        assert not got["dh0"][0].any() and not got["dc0"][0].any()
        bad = float_failures(float_tensors(got), ex, em, figure={
            "kind": "core_float", "lstm_size": lstm_size, "routes": "+".join(routes) or "off",
            "mode": mode})
        assert not bad, bad


def _capture_fc_input(model, monkeypatch, replace=None):
    """Record the tensor entering `fc` (default route) or `trunk_fc` (fused
    route) during the next forwards, or put `replace` in its place."""
    from moolib_amd.ops import fc as fc_ops

    seen = []
    op = fc_ops.trunk_fc

    def pre_hook(module, args):
        seen.append(args[0])
        return None if replace is None else (replace,)

    def trunk_fc(x, *a, **kw):
        seen.append(x)
        return op(x if replace is None else replace, *a, **kw)

    handle = model.fc.register_forward_pre_hook(pre_hook)
    monkeypatch.setattr(fc_ops, "trunk_fc", trunk_fc)
    return seen, handle


@gpu
@requires_gpu
class TestRouteRelations:
    @pytest.mark.parametrize("mode", ["a", "b"])
    @pytest.mark.parametrize("lstm_size", WIDTHS)
    def test_recurrent_flag_changes_dw_hh_only(self, lstm_size, mode, calls):
        """ops/lstm.py: with native_whh "all outputs and gradients but dW are
        bit-identical to the default". Through the model: outputs, state, dh0,
        dc0, the gradient of every parameter from `fc` on but dW_hh, and the
        gradient handed to the trunk are `torch.equal`; dW_hh is within the
        float bound. The 30 section gradients are functions of that one
        gradient, but two runs of the conv weight-gradient kernels (float
        atomics in the project's first-conv kernel, the vendor's in the rest)
        do not repeat bit for bit, flag or no flag, so they are held to the
        float bound and how many were equal is printed. Under no_grad
        everything returned is equal (at 128 / 512 the forward-only scan on
        pack_whh's operand against the one on pack_mfma_b's)."""
        _, inputs, core, grads = case(lstm_size)
        res = {}
        for routes in (OFF, ("core_recurrent",)):
            model = build_model(lstm_size, mode, routes)
            calls.clear()
            out = run_model(model, mode, inputs, core, grads)
            res[routes, "grad"] = dict(float_tensors(out), d_trunk=out["d_trunk"])
            assert calls == expected_calls(lstm_size, routes), calls
            if routes == OFF:  # the same model once more: what repeats without any flag
                res["rerun"] = float_tensors(run_model(model, mode, inputs, core, grads))
            calls.clear()
            res[routes, "no_grad"] = float_tensors(run_model(model, mode, inputs, core,
                                                             no_grad=True))
            assert calls == expected_calls(lstm_size, routes, no_grad=True), calls
        off, on = res[OFF, "grad"], res[("core_recurrent",), "grad"]
        dw = "grad core.weight_hh_l0"
        sections = ["grad " + k for k in TR.SECTION_PARAMS]
        assert set(off) == set(on) and len(on) == 47 and on["d_trunk"].shape == (9, 3872)
        differ = [k for k in off if k != dw and k not in sections and not torch.equal(off[k], on[k])]
        assert not differ, differ
        _figure(kind="core_recurrent_dw", lstm_size=lstm_size, mode=mode,
                equal=torch.equal(off[dw], on[dw]),
                diff=(off[dw].double() - on[dw].double()).abs().max().item(),
                sections_equal=sum(torch.equal(off[k], on[k]) for k in sections),
                sections_equal_rerun=sum(torch.equal(off[k], res["rerun"][k]) for k in sections),
                others_equal_rerun=all(torch.equal(off[k], res["rerun"][k])
                                       for k in res["rerun"] if k not in sections))
        ex, em = exact_ref(lstm_size), emul_ref(lstm_size, mode)
        assert not float_failures(on, ex, em, only=[dw] + sections)
        off, on = res[OFF, "no_grad"], res[("core_recurrent",), "no_grad"]
        assert sorted(on) == sorted(OUTPUTS)
        differ = [k for k in off if not torch.equal(off[k], on[k])]
        assert not differ, differ

    @pytest.mark.parametrize("mode", ["a", "b"])
    @pytest.mark.parametrize("routes", [OFF, ALL_ON], ids=_ids)
    @pytest.mark.parametrize("lstm_size", [128, 512])
    def test_forward_only_scan_in_the_model(self, lstm_size, routes, mode, calls, monkeypatch):
        """Grad-mode forward against the no_grad forward of the same model
        from the FC input on (the no-grad trunk rounds a block once where the
        autograd path rounds twice, so the trunk's own values are not promised
        to agree): logits, baseline, hT and cT must be `torch.equal`."""
        _, inputs, core, _ = case(lstm_size)
        model = build_model(lstm_size, mode, routes)
        seen, handle = _capture_fc_input(model, monkeypatch)
        try:
            with_grad = run_model(model, mode, inputs, core)
        finally:
            handle.remove()
        (x,) = seen
        want = expected_calls(lstm_size, routes)
        want.pop("lstm_whh_grad", None)  # no backward here
        assert calls == want and calls["lstm_wide_fwd_saving"] == 1, calls
        calls.clear()
        seen, handle = _capture_fc_input(model, monkeypatch, replace=x.detach())
        try:
            without = run_model(model, mode, inputs, core, no_grad=True)
        finally:
            handle.remove()
        assert len(seen) == 1 and calls == expected_calls(lstm_size, routes, no_grad=True), calls
        differ = [k for k in OUTPUTS if not torch.equal(with_grad[k], without[k])]
        assert not differ, differ


@gpu
@requires_gpu
class TestActorStepping:
    @pytest.mark.parametrize("routes", [OFF, ALL_ON], ids=_ids)
    @pytest.mark.parametrize("lstm_size", WIDTHS)
    def test_three_calls_against_one_sequence(self, lstm_size, routes, calls):
        """The actor's use of the core, mode (a), no_grad: three T=1 calls
        carrying the returned fp32 state, against the reference of the T=3
        sequence; with every flag on, `fused_actor_sections` too."""
        _, inputs, core, _ = case(lstm_size)
        actor = routes == ALL_ON
        model = build_model(lstm_size, "a", routes, actor_sections=actor)
        state = tuple(s.cuda() for s in model.initial_state(batch_size=3))
        assert all(s.dtype == torch.float32 for s in state)
        state = tuple(c.cuda().to(s.dtype) for c, s in zip(core, state))
        inputs = {k: v.cuda() for k, v in inputs.items()}
        steps, states, first_state = [], [], state
        with torch.no_grad():
            for t in range(3):
                out, state = model({k: v[t : t + 1] for k, v in inputs.items()}, state)
                assert state[0].dtype == state[1].dtype == torch.float32
                steps.append(out)
                states.append(state)
            whole, whole_state = model(inputs, first_state)
            # row 0 is done at t=0: its first step must not see its initial state
            other = tuple(s.clone() for s in first_state)
            other[0][0, 0] = 0.75
            other[1][0, 0] = -1.3
            again, again_state = model({k: v[:1] for k, v in inputs.items()}, other)
        assert calls == expected_calls(lstm_size, routes, no_grad=True, actor_sections=actor,
                                       forwards=5), calls
        got = {k: torch.cat([o[k] for o in steps]).cpu() for k in ("policy_logits", "baseline")}
        got["hT"], got["cT"] = state[0][0].cpu(), state[1][0].cpu()
        one = {k: whole[k].cpu() for k in ("policy_logits", "baseline")}
        one["hT"], one["cT"] = whole_state[0][0].cpu(), whole_state[1][0].cpu()
        ex, em = exact_ref(lstm_size), emul_ref(lstm_size, "a", routes)
        fig = {"lstm_size": lstm_size, "routes": "+".join(routes) or "off"}
        _figure(kind="core_stepping_equal", **fig,
                **{k: torch.equal(got[k], one[k]) for k in OUTPUTS})
        assert not float_failures(got, ex, em, figure=dict(fig, kind="core_stepping"),
                                  only=OUTPUTS)
        assert not float_failures(one, ex, em, only=OUTPUTS)
        for k in ("policy_logits", "baseline"):
            assert torch.equal(again[k][0, 0], steps[0][k][0, 0]), k
        for s, s0 in zip(again_state, states[0]):
            assert torch.equal(s[0, 0], s0[0, 0])
