"""Fused flat Adam step (ops.flat_adam, optim.FlatAdam, the two learners'
`fused_optimizer` flag): docs/KERNEL_TESTS.md, "Optimizer".

The float64 reference (tests/flat_adam_refs.py) is written from the
definition and itself checked against clip_grad_norm_ + torch.optim.Adam on
float64 parameters. Integer-valued inputs make every intermediate exact in
fp32, so the eager path and the kernels must equal the reference bit for bit;
random-float inputs are held to `4 max(e_ref, 2^-24 max|ref|)` per tensor,
where e_ref is the error of the fp32 eager path on the same inputs (plus one
bf16 rounding, 2^-8 |ref|, for the shadow weights).
"""
import copy
import functools
import json

import pytest
import torch

import flat_adam_refs as R
from moolib_amd.ops import flat_adam as ops
from moolib_amd.optim import FlatAdam

gpu = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

U = 2.0 ** -24
P = ops.PASS_ELEMENTS
SMALL_N = [1, 2, 3, 4, 5, 7, 255, 256, 257, 1023, 1025]
KERNEL_N = SMALL_N + [P - 1, P, P + 1, 2 ** 21 + 3]
PREMISE_N = [144, 257, 1025, 2 ** 21 + 3]
FLOAT_N = 1025


def _figure(**kw):
    """One machine-readable line per measured figure (shown with pytest -s)."""
    print("KERNEL_EDGES_FIGURE " + json.dumps(kw))


def int_kinds(N):
    return ["none", "clip" if N >= R.INT_CLIP_MIN_N else "clamp"]


def run_op(device, p, g, m, v, step, lr, beta1, beta2, eps, max_norm, shadow=True,
           sentinels=True):
    """One flat_adam_step on copies of the fp32 inputs; everything back on the
    CPU. Outputs the op must write are pre-filled with sentinels."""
    N = p.numel()
    dp, dg, dm, dv = (x.clone().to(device) for x in (p, g, m, v))
    dstep = torch.tensor(step, dtype=torch.int64, device=device)
    dlr = torch.tensor(lr, dtype=torch.float32, device=device)
    dshadow = torch.full((N,), float("nan"), dtype=torch.bfloat16, device=device) if shadow else None
    ws = None
    if torch.device(device).type == "cuda":
        ws = ops.new_workspace(device)
        if sentinels:
            ws.partial.fill_(-12345.0)
            ws.norm.fill_(float("nan"))
            ws.step_next.fill_(-777)
    norm = ops.flat_adam_step(dp, dg, dm, dv, dstep, dlr, beta1, beta2, eps, shadow=dshadow,
                              max_norm=max_norm, workspace=ws)
    assert norm.dim() == 0 and norm.dtype == torch.float32
    assert torch.equal(dg.cpu(), g), "the gradient must be left as it is"
    out = dict(p=dp.cpu(), m=dm.cpu(), v=dv.cpu(), norm=norm.cpu(), step=dstep.cpu())
    if shadow:
        out["shadow"] = dshadow.cpu()
    return out


def run_int(device, N, kind):
    p, g, max_norm = R.integer_case(N, kind)
    z = torch.zeros(N)
    return run_op(device, p, g, z, z, 0, R.INT["lr"], R.INT["beta1"], R.INT["beta2"],
                  R.INT["eps"], max_norm)


def check_int_equal(out, N, kind):
    ref = R.integer_ref(N, kind)
    for k in ("p", "m", "v"):
        assert torch.equal(out[k], getattr(ref, k).float()), k
        assert torch.equal(out[k].double(), getattr(ref, k)), k
    assert torch.equal(out["shadow"], ref.p.to(torch.bfloat16))
    # S is an exact integer in any order; norm = (float) sqrt(S), IEEE double sqrt
    assert torch.equal(out["norm"], torch.tensor(ref.norm, dtype=torch.float64).float())
    if kind == "clip":
        assert float(out["norm"]) == 64.0
    assert int(out["step"]) == 1 == ref.t


@functools.lru_cache(maxsize=None)
def eager_float(N, scale, eps, max_norm):
    """The fp32 eager path on the CPU and its error against float64."""
    p, g, m, v = R.float_case(N, scale, eps, max_norm)
    out = run_op("cpu", p, g, m, v, R.FLOAT_STEP, R.FLOAT["lr"], R.FLOAT["beta1"],
                 R.FLOAT["beta2"], eps, max_norm)
    ref = R.float_ref(N, scale, eps, max_norm)
    return out, errors(out, ref)


def errors(out, ref):
    e = {k: float((out[k].double() - getattr(ref, k)).abs().max()) for k in ("p", "m", "v")}
    e["norm"] = abs(float(out["norm"]) - ref.norm)
    return e


def bounds(e_ref, ref):
    """4 max(e_ref, 2^-24 max|ref|) per tensor."""
    b = {k: 4.0 * max(e_ref[k], U * float(getattr(ref, k).abs().max())) for k in ("p", "m", "v")}
    b["norm"] = 4.0 * max(e_ref["norm"], U * ref.norm)
    return b


def check_float(out, ref, e_ref, label):
    """Every tensor within its bound of the float64 reference; the shadow
    within that plus one bf16 rounding. Returns the worst error / bound."""
    b = bounds(e_ref, ref)
    e = errors(out, ref)
    ratios = {k: e[k] / b[k] for k in b}
    if "shadow" in out:
        err = (out["shadow"].double() - ref.p).abs()
        ratios["shadow"] = float((err / (b["p"] + 2.0 ** -8 * ref.p.abs())).max())
    _figure(test=label, **{k: round(r, 4) for k, r in ratios.items()})
    for k, r in ratios.items():
        assert r <= 1.0, (label, k, r)
    return ratios


FLOAT_CASES = [(s, e, mn) for s in R.FLOAT_SCALES for e in R.FLOAT_EPS for mn in R.FLOAT_MAX_NORM]


# ================================================================ CPU tests


class TestReference:
    @pytest.mark.parametrize("k", [1, 2, 7])
    @pytest.mark.parametrize("max_norm", [None, 0.5])
    @pytest.mark.parametrize("N", [1, 5, 1000])
    def test_agrees_with_torch_float64(self, N, max_norm, k):
        gen = torch.Generator().manual_seed(N + k)
        sizes = R.split_sizes(N, k)
        p0 = torch.randn(N, generator=gen, dtype=torch.float64)
        params = [torch.nn.Parameter(c.clone()) for c in p0.split(sizes)]
        opt = torch.optim.Adam(params, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, foreach=False)
        p, m, v = p0, torch.zeros(N, dtype=torch.float64), torch.zeros(N, dtype=torch.float64)
        for step in range(5):
            g = torch.randn(N, generator=gen, dtype=torch.float64)
            for q, c in zip(params, g.split(sizes)):
                q.grad = c.clone()
            want_norm = None
            if max_norm is not None:
                want_norm = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
            opt.step()
            out = R.flat_adam_ref(p, g, m, v, step, 1e-2, 0.9, 0.999, 1e-8, max_norm,
                                  coef_fp32=False)
            p, m, v = out.p, out.m, out.v
            got = torch.cat([q.detach().reshape(-1) for q in params])
            assert float((got - p).abs().max()) <= 1e-12
            if want_norm is not None:
                assert abs(want_norm - out.norm) <= 1e-12 * max(1.0, out.norm)
                # the definition's fp32 coefficient is the same number rounded
                c32 = R.clip_coef(out.norm, max_norm, fp32=True)
                assert abs(c32 - out.coef) <= 4 * U * out.coef
            nonempty = [(q, opt.state[q]) for q in params if q.numel()]
            got_m = torch.cat([s["exp_avg"].reshape(-1) for _, s in nonempty])
            got_v = torch.cat([s["exp_avg_sq"].reshape(-1) for _, s in nonempty])
            assert float((got_m - m).abs().max()) <= 1e-12
            assert float((got_v - v).abs().max()) <= 1e-12


class TestIntegerExactCPU:
    @pytest.mark.parametrize("N", PREMISE_N)
    def test_premise(self, N):
        """With these inputs every value is exact in fp32 in any order, and
        fp32 torch Adam (both foreach settings) equals float64 bit for bit."""
        for kind in ("none", "clip"):
            p, g, max_norm = R.integer_case(N, kind)
            ref = R.integer_ref(N, kind)
            gh = g.double() * ref.coef
            if kind == "clip":
                assert int((g.abs() == 2).sum()) == 84 and int((g.abs() == 6).sum()) == 50
                assert int((g.abs() == 14).sum()) == 10 and int((g != 0).sum()) == 144
                assert float((g.double() ** 2).sum()) == 4096.0
                assert ref.norm == 64.0 and ref.coef == 0.5
                assert torch.tensor(64.0) + 1e-6 == 64.0  # fp32
            else:
                assert ref.coef == 1.0
            assert set(gh.abs().tolist()) <= {0.0, 1.0, 3.0, 7.0}
            assert torch.equal(ref.m, gh / 2) and torch.equal(ref.v, gh * gh / 4)
            denom = ref.v.sqrt() / 0.5 + 1.0
            assert set(denom.tolist()) <= {1.0, 2.0, 4.0, 8.0}
            assert torch.equal(ref.p, p.double() - 0.25 * ref.m / denom)
            for t in (ref.p, ref.m, ref.v):  # exact in fp32
                assert torch.equal(t.float().double(), t)
            # the bf16 rounding is exercised: ties and inexact values are common
            # (the clipped case moves only 144 positions, 84 of them by 1/16,
            # which bf16 holds next to any |p| <= 8: it cannot reach a quarter)
            inexact = ref.p.to(torch.bfloat16).double() != ref.p
            if kind == "none":
                assert float(inexact.double().mean()) >= 0.25
            else:
                assert int(inexact.sum()) >= 1
            for foreach in (False, True):
                q = torch.nn.Parameter(p.clone())
                q.grad = g.clone()
                opt = torch.optim.Adam([q], lr=R.INT["lr"], betas=(0.5, 0.75), eps=1.0,
                                       foreach=foreach)
                if max_norm is not None:
                    norm = torch.nn.utils.clip_grad_norm_([q], max_norm)
                    assert float(norm) == 64.0
                opt.step()
                assert torch.equal(q.detach().double(), ref.p)
                assert torch.equal(opt.state[q]["exp_avg"].double(), ref.m)
                assert torch.equal(opt.state[q]["exp_avg_sq"].double(), ref.v)

    def test_clamp_premise(self):
        for N in SMALL_N:
            if N < R.INT_CLIP_MIN_N:
                assert R.integer_ref(N, "clamp").coef == 1.0

    @pytest.mark.parametrize("N", KERNEL_N)
    def test_eager_equals_reference(self, N):
        for kind in int_kinds(N):
            check_int_equal(run_int("cpu", N, kind), N, kind)


def float_scales(N, scale, eps, max_norm):
    """First-order sizes of the fp32 rounding errors of one step, from the
    reference's own values: every output is a handful of fp32 operations on
    terms of these magnitudes (u = 2^-24 each)."""
    p, g, m, v = (x.double() for x in R.float_case(N, scale, eps, max_norm))
    ref = R.float_ref(N, scale, eps, max_norm)
    gh = g * ref.coef
    bc1 = 1 - R.FLOAT["beta1"] ** ref.t
    bc2 = 1 - R.FLOAT["beta2"] ** ref.t
    denom = ref.v.sqrt() / bc2 ** 0.5 + eps
    return dict(
        m=float((gh.abs() + m.abs()).max()),
        v=float((v + gh * gh).max()),
        p=float(p.abs().max() + (R.FLOAT["lr"] / bc1 * (gh.abs() + m.abs() + ref.m.abs()) / denom).max()),
        norm=ref.norm,
    )


class TestFloatCPU:
    @pytest.mark.parametrize("scale,eps,max_norm", FLOAT_CASES)
    def test_eager_error_is_rounding(self, scale, eps, max_norm):
        """e_ref, the yardstick of the kernel tests, is itself no more than a
        few roundings: 16 u times the magnitudes that enter each output."""
        out, e_ref = eager_float(FLOAT_N, scale, eps, max_norm)
        s = float_scales(FLOAT_N, scale, eps, max_norm)
        ref = R.float_ref(FLOAT_N, scale, eps, max_norm)
        _figure(test="eager_float", scale=scale, eps=eps, max_norm=max_norm,
                **{k: round(e_ref[k] / (16 * U * s[k]), 4) for k in s})
        for k in s:
            assert e_ref[k] <= 16 * U * s[k], (k, e_ref[k], s[k])
        assert int(out["step"]) == R.FLOAT_STEP + 1
        err = (out["shadow"].double() - ref.p).abs()
        assert bool((err <= e_ref["p"] + 2.0 ** -8 * ref.p.abs()).all())

    def test_nonfinite_gradient_propagates(self):
        p, g, m, v = (x.clone() for x in R.float_case(FLOAT_N, 1.0, 1e-8, 40.0))
        g[3] = float("inf")
        out = run_op("cpu", p, g, m, v, 3, 6e-4, 0.9, 0.999, 1e-8, 40.0)
        assert float(out["norm"]) == float("inf") and int(out["step"]) == 4
        assert bool(torch.isnan(out["p"][3])) and bool(torch.isnan(out["shadow"][3].float()))


class TestArgumentsCPU:
    def _args(self, N=8):
        z = lambda: torch.zeros(N)
        return [z(), z(), z(), z(), torch.tensor(0), torch.tensor(1e-3)]

    @pytest.mark.parametrize("bad", ["dtype", "length", "step", "lr", "beta", "eps", "max_norm",
                                     "shadow", "empty", "align"])
    def test_op_rejects(self, bad):
        a, kw = self._args(), {}
        if bad == "dtype":
            a[1] = a[1].double()
        elif bad == "length":
            a[2] = torch.zeros(9)
        elif bad == "step":
            a[4] = torch.tensor(0.0)
        elif bad == "lr":
            a[5] = torch.tensor(1e-3, dtype=torch.float64)
        elif bad == "beta":
            kw["beta1"] = 1.0
        elif bad == "eps":
            kw["eps"] = -1.0
        elif bad == "max_norm":
            kw["max_norm"] = 0.0
        elif bad == "shadow":
            kw["shadow"] = torch.zeros(8)
        elif bad == "empty":
            a[:4] = [torch.zeros(0) for _ in range(4)]
        elif bad == "align":
            a[0] = torch.zeros(9)[1:]
        with pytest.raises(ValueError, match="flat_adam_step"):
            ops.flat_adam_step(*a, **kw)

    @pytest.mark.parametrize("bad", ["groups", "weight_decay", "amsgrad", "maximize", "beta",
                                     "eps", "max_grad_norm", "group_weight_decay", "dtype"])
    def test_optimizer_rejects(self, bad):
        a = torch.nn.Parameter(torch.zeros(3))
        b = torch.nn.Parameter(torch.zeros(2))
        params, kw = [a, b], {}
        if bad == "groups":
            params = [{"params": [a]}, {"params": [b]}]
        elif bad == "group_weight_decay":
            params = [{"params": [a, b], "weight_decay": 0.1}]
        elif bad == "dtype":
            params = [a, torch.nn.Parameter(torch.zeros(2, dtype=torch.float64))]
        elif bad == "beta":
            kw["betas"] = (0.9, 1.0)
        elif bad == "eps":
            kw["eps"] = -1e-8
        elif bad == "max_grad_norm":
            kw["max_grad_norm"] = 0.0
        else:
            kw[bad] = 0.1 if bad == "weight_decay" else True
        with pytest.raises(ValueError, match="FlatAdam"):
            FlatAdam(params, lr=1e-3, **kw)


# ---------------------------------------------------------------- optimizer


def make_models(device="cpu", seed=5):
    torch.manual_seed(seed)
    a = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Tanh(), torch.nn.Linear(5, 3))
    a.to(device)
    return a, copy.deepcopy(a)


def seeded_grads(params, seed, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    return [scale * torch.randn(p.shape, generator=gen) for p in params]


def set_grads(params, grads):
    with torch.no_grad():
        for p, g in zip(params, grads):
            if p.grad is None:
                p.grad = g.clone().to(p.device)
            else:
                p.grad.copy_(g)


def flat(tensors):
    return torch.cat([t.detach().reshape(-1).cpu() for t in tensors])


def flat_state(opt, params, key):
    return torch.cat([opt.state_dict()["state"][i][key].reshape(-1).cpu() for i in range(len(params))])


HYPER = dict(lr=6e-4, betas=(0.9, 0.999), eps=1e-8)
CLIP = 0.5


def ref_trajectory(params0, grads_per_step, max_norm=CLIP, lr=None):
    """float64 reference over several steps; lr may be a list per step."""
    p = flat(list(params0)).double()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    outs = []
    for s, grads in enumerate(grads_per_step):
        step_lr = HYPER["lr"] if lr is None else lr[s]
        out = R.flat_adam_ref(p, flat(grads), m, v, s, step_lr, *HYPER["betas"], HYPER["eps"],
                              max_norm)
        p, m, v = out.p, out.m, out.v
        outs.append(out)
    return outs


def eager_trajectory(params0, grads_per_step, max_norm=CLIP, lr=None):
    """The fp32 eager op on the CPU over the same steps: e_ref per step."""
    params0 = list(params0)
    p = flat(params0).clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    step, dlr = torch.tensor(0), torch.tensor(HYPER["lr"])
    refs = ref_trajectory(params0, grads_per_step, max_norm, lr)
    errs = []
    for s, grads in enumerate(grads_per_step):
        if lr is not None:
            dlr.fill_(lr[s])
        norm = ops.flat_adam_step(p, flat(grads), m, v, step, dlr, *HYPER["betas"], HYPER["eps"],
                                  max_norm=max_norm)
        errs.append(errors(dict(p=p, m=m, v=v, norm=norm), refs[s]))
    return refs, errs


def within(got, ref, e_ref, what):
    bound = 4.0 * max(e_ref, U * float(ref.abs().max()))
    err = float((got.double().cpu() - ref).abs().max())
    assert err <= bound, (what, err, bound)
    return err / bound


class TestOptimizerCPU:
    def test_views_and_zero_grad(self):
        model, _ = make_models()
        params = list(model.parameters())
        before = [p.detach().clone() for p in params]
        opt = FlatAdam(params, max_grad_norm=CLIP, **HYPER)
        for p, b in zip(params, before):
            assert torch.equal(p.detach(), b)
        model(torch.randn(4, 7)).sum().backward()
        assert float(opt._flat_g.abs().sum()) > 0  # autograd landed in the flat buffer
        ptrs = [p.grad.data_ptr() for p in params]
        for set_to_none in (True, False):
            opt.zero_grad(set_to_none=set_to_none)
            assert [p.grad.data_ptr() for p in params] == ptrs
            assert all(p.grad is not None and float(p.grad.abs().sum()) == 0 for p in params)
        off = 0
        for p in params:
            assert p.data_ptr() == opt._flat_p.data_ptr() + 4 * off
            assert p.grad.data_ptr() == opt._flat_g.data_ptr() + 4 * off
            off += p.numel()

    def test_steps_match_reference_and_shadow(self):
        model, _ = make_models()
        params = list(model.parameters())
        shadow = [torch.nn.Parameter(p.detach().to(torch.bfloat16)) for p in params]
        grads = [seeded_grads(params, 40 + s) for s in range(3)]
        refs, errs = eager_trajectory(params, grads)
        opt = FlatAdam(params, max_grad_norm=CLIP, shadow_params=shadow, **HYPER)
        versions = [p._version for p in params + shadow]
        for s in range(3):
            set_grads(params, grads[s])
            norm = opt.step()
            assert norm.dim() == 0 and abs(float(norm) - refs[s].norm) <= 4 * U * refs[s].norm
        within(flat(params), refs[-1].p, errs[-1]["p"], "p")
        assert torch.equal(flat(shadow), flat(params).to(torch.bfloat16))
        assert all(p._version > v0 for p, v0 in zip(params + shadow, versions))
        assert int(opt._step) == 3

    def test_adopts_flat_buffers(self):
        from moolib_amd.impala import flatten_master_shadow

        model, _ = make_models()
        fwd = copy.deepcopy(model).to(torch.bfloat16)
        mp, sp = list(model.parameters()), list(fwd.parameters())
        fm, fs, g32, _ = flatten_master_shadow(mp, sp)
        opt = FlatAdam(mp, max_grad_norm=CLIP, shadow_params=sp, flat=(fm, g32, fs), **HYPER)
        assert opt._flat_p is fm and opt._flat_g is g32 and opt._flat_shadow is fs
        grads = [seeded_grads(mp, 77)]
        set_grads(mp, grads[0])
        opt.step()
        refs, errs = eager_trajectory(make_models()[0].parameters(), grads)
        within(fm, refs[0].p, errs[0]["p"], "p")
        assert torch.equal(fs, fm.to(torch.bfloat16))
        with pytest.raises(ValueError, match="FlatAdam"):
            FlatAdam(list(make_models()[0].parameters()), flat=(fm, g32), **HYPER)

    @pytest.mark.parametrize("direction", ["adam_to_flat", "flat_to_adam"])
    def test_state_dict_exchange(self, direction):
        """3 steps in one optimizer, its state into the other, the 4th step
        there: within the float bound of 4 reference steps."""
        src_model, dst_model = make_models()
        sp, dp = list(src_model.parameters()), list(dst_model.parameters())
        grads = [seeded_grads(sp, 60 + s) for s in range(4)]
        refs, errs = eager_trajectory(sp, grads)

        def adam(params):
            return torch.optim.Adam(params, foreach=False, **HYPER)

        def fused(params):
            return FlatAdam(params, max_grad_norm=CLIP, **HYPER)

        src, dst = (adam(sp), fused(dp)) if direction == "adam_to_flat" else (fused(sp), adam(dp))

        def step(opt, params, g):
            set_grads(params, g)
            if isinstance(opt, torch.optim.Adam):
                torch.nn.utils.clip_grad_norm_(params, CLIP)
            opt.step()

        for s in range(3):
            step(src, sp, grads[s])
        ptrs = [p.data_ptr() for p in dp]
        with torch.no_grad():
            for q, p in zip(dp, sp):
                q.copy_(p)
        dst.load_state_dict(copy.deepcopy(src.state_dict()))
        assert [p.data_ptr() for p in dp] == ptrs, "loading must not replace the views"
        step(dst, dp, grads[3])
        within(flat(dp), refs[3].p, errs[3]["p"], "p")
        within(flat_state(dst, dp, "exp_avg"), refs[3].m, errs[3]["m"], "m")
        within(flat_state(dst, dp, "exp_avg_sq"), refs[3].v, errs[3]["v"], "v")
        sd = dst.state_dict()
        assert set(sd["state"][0]) >= {"step", "exp_avg", "exp_avg_sq"}
        assert all(float(sd["state"][i]["step"]) == 4.0 for i in range(len(dp)))
        assert sd["param_groups"][0]["params"] == list(range(len(dp)))

    def test_lambda_lr_halves_the_update(self):
        """With m = v = 0 before the step the update is lr times a function of
        the gradient alone, so half the lr is half the update."""
        deltas = []
        for halve in (False, True):
            model, _ = make_models()
            params = list(model.parameters())
            opt = FlatAdam(params, **HYPER)
            sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: 0.5 ** e)
            grads = [seeded_grads(params, 90), seeded_grads(params, 91)]
            if halve:  # burn one scheduler epoch without moving the moments
                set_grads(params, [torch.zeros_like(g) for g in grads[0]])
                opt.step()
                sched.step()
                with torch.no_grad():
                    opt._step.zero_()
                assert opt.param_groups[0]["lr"] == HYPER["lr"] / 2
            before = flat(params).double()
            set_grads(params, grads[1])
            opt.step()
            assert float(opt._lr) == pytest.approx(opt.param_groups[0]["lr"], rel=1e-7)
            deltas.append(flat(params).double() - before)
        full, half = deltas
        assert float(full.abs().max()) > 0
        assert float((half - full / 2).abs().max()) <= 4 * U * float(flat(params).abs().max())


# ------------------------------------------------------------------ learners


class TinyNet(torch.nn.Module):
    """CartPole-sized stand-in with AtariNet's forward contract: [T,B,4] float
    state, an LSTM core reset where done, policy_logits / baseline heads."""

    def __init__(self, num_actions=3):
        super().__init__()
        self.num_actions = num_actions
        self.fc = torch.nn.Linear(4 + 1 + num_actions, 8)
        self.core = torch.nn.LSTM(8, 8)
        self.policy = torch.nn.Linear(8, num_actions)
        self.baseline = torch.nn.Linear(8, 1)

    def initial_state(self, batch_size=1):
        return tuple(torch.zeros(1, batch_size, 8) for _ in range(2))

    def forward(self, inputs, core_state):
        T, B = inputs["reward"].shape
        onehot = torch.nn.functional.one_hot(inputs["prev_action"], self.num_actions).float()
        x = torch.cat([inputs["state"], inputs["reward"].unsqueeze(-1), onehot], dim=-1)
        x = torch.relu(self.fc(x))
        outs = []
        for t in range(T):
            nd = (~inputs["done"][t]).float().view(1, B, 1)
            core_state = tuple(nd * s for s in core_state)
            o, core_state = self.core(x[t:t + 1], core_state)
            outs.append(o)
        y = torch.cat(outs)
        out = {"policy_logits": self.policy(y), "baseline": self.baseline(y).squeeze(-1)}
        return out, core_state


def r2d2_batch(T=6, B=4, A=3):
    g = torch.Generator().manual_seed(4)
    return {
        "state": torch.randn(T, B, 4, generator=g),
        "reward": torch.randn(T, B, generator=g),
        "done": torch.rand(T, B, generator=g) < 0.15,
        "prev_action": torch.randint(0, A, (T, B), generator=g),
        "action": torch.randint(0, A, (T, B), generator=g),
    }


def check_r2d2_learn(device):
    """One R2D2Learner.learn with the flag on: new parameters and grad_norm
    within the float bound of flat_adam_ref on the snapshot around it."""
    from moolib_amd.r2d2 import R2D2Config, R2D2Learner

    torch.manual_seed(0)
    cfg = R2D2Config(lr=1e-2, burn_in=1, n_step=2, grad_clip=0.05, fused_optimizer=True)
    learner = R2D2Learner(TinyNet(), cfg, device, autocast=False)
    assert isinstance(learner.optimizer, FlatAdam)
    params = list(learner.online.parameters())
    before = flat(params)
    metrics, priorities = learner.learn(r2d2_batch(), torch.ones(4))
    grads = flat([p.grad for p in params])  # left unclipped by the fused step
    N = before.numel()
    z = torch.zeros(N)
    ref = R.flat_adam_ref(before, grads, z, z, 0, cfg.lr, 0.9, 0.999, 1e-3, cfg.grad_clip)
    assert ref.coef < 1.0, "the case must clip"
    eager = run_op("cpu", before, grads, z, z, 0, cfg.lr, 0.9, 0.999, 1e-3, cfg.grad_clip)
    e_ref = errors(eager, ref)
    r_p = within(flat(params), ref.p, e_ref["p"], "p")
    r_n = within(metrics["grad_norm"].reshape(1), torch.tensor([ref.norm], dtype=torch.float64),
                 e_ref["norm"], "grad_norm")
    _figure(test="r2d2_learn", device=str(device), p=round(r_p, 4), grad_norm=round(r_n, 4))
    assert float((flat(params) - before).abs().max()) > 0
    assert priorities.shape == (4,) and int(learner.optimizer._step) == 1


def make_impala_peer(device, **kw):
    import moolib_amd
    from moolib_amd.envs import SyntheticAtariEnv
    from moolib_amd.impala import ImpalaConfig, ImpalaPeer

    rpc = moolib_amd.Rpc()
    rpc.set_name("broker")
    broker = moolib_amd.Broker(rpc)
    addr = rpc.listen("127.0.0.1:0")[0]
    base = dict(num_actions=6, actor_batch_size=4, num_actor_batches=2, num_actor_cpus=2,
                batch_size=4, unroll_length=5, virtual_batch_size=4, device=device, connect=addr,
                total_steps=1e4, seed=3, fused_optimizer=True)
    base.update(kw)
    cfg = ImpalaConfig(**base)
    torch.manual_seed(11)
    peer = ImpalaPeer(cfg, lambda: SyntheticAtariEnv(num_actions=6), broker=broker)
    return peer, broker


def close_peer(peer):
    import gc

    for name in list(vars(peer)):
        setattr(peer, name, None)
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def impala_ref_step(peer, params, step, seed):
    """Seed the master gradients, take one step_optimizer, and hold the new
    parameters to flat_adam_ref on the snapshot."""
    cfg = peer.cfg
    before = flat(params)
    grads = seeded_grads(params, seed, scale=0.05)
    set_grads(params, grads)
    lr = peer.optimizer.param_groups[0]["lr"]
    m = flat_state(peer.optimizer, params, "exp_avg")
    v = flat_state(peer.optimizer, params, "exp_avg_sq")
    peer.step_optimizer()
    # the step ran at the lr the scheduler had set before it, replays included
    assert float(peer.optimizer._lr) == pytest.approx(lr, rel=1e-7)
    assert peer.optimizer.param_groups[0]["lr"] < lr
    args = (step, lr, cfg.adam_beta1, cfg.adam_beta2, cfg.adam_eps, cfg.grad_norm_clipping)
    ref = R.flat_adam_ref(before, flat(grads), m, v, *args)
    eager = run_op("cpu", before, flat(grads), m, v, *args)
    e_ref = errors(eager, ref)
    ratio = within(flat(params), ref.p, e_ref["p"], "p at step %d" % step)
    assert float((flat(params) - before).abs().max()) > 0
    return ref, ratio


class TestLearnersCPU:
    def test_r2d2_learn(self):
        check_r2d2_learn("cpu")

    def test_r2d2_flag_off_is_adam(self):
        from moolib_amd.r2d2 import R2D2Config, R2D2Learner

        learner = R2D2Learner(TinyNet(), R2D2Config(), "cpu")
        assert type(learner.optimizer) is torch.optim.Adam

    @pytest.mark.timeout(120)
    def test_impala_step_optimizer(self, monkeypatch):
        monkeypatch.delenv("MOOLIB_AMD_FUSED_OPT", raising=False)
        peer, broker = make_impala_peer("cpu", autocast_bf16=False, grad_norm_clipping=1.0)
        try:
            assert isinstance(peer.optimizer, FlatAdam) and peer.scheduler is not None
            assert not peer._graph_opt
            params = [p for p in peer.model.parameters() if p.requires_grad]
            lr0 = peer.optimizer.param_groups[0]["lr"]
            ref, _ = impala_ref_step(peer, params, 0, seed=21)
            assert ref.coef < 1.0, "the case must clip"
            assert peer.model_version == 1
            assert peer.optimizer.param_groups[0]["lr"] < lr0  # the scheduler wraps FlatAdam
            impala_ref_step(peer, params, 1, seed=22)
            # the state a joining peer receives loads into an eager Adam
            state = peer.save_state()
            adam = torch.optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in params],
                                    foreach=True)
            adam.load_state_dict(state["optimizer"])
            assert float(adam.state_dict()["state"][0]["step"]) == 2.0
            peer.load_state(state)
            assert int(peer.optimizer._step) == 2
            # and an eager leader's state loads into the fused peer
            for q in adam.param_groups[0]["params"]:
                q.grad = torch.ones_like(q)
            adam.step()
            ptrs = [p.data_ptr() for p in params]
            peer.load_state({"optimizer": adam.state_dict(), "scheduler": None,
                             "model_version": 7})
            assert int(peer.optimizer._step) == 3 and peer.model_version == 7
            assert [p.data_ptr() for p in params] == ptrs
            assert torch.equal(flat_state(peer.optimizer, params, "exp_avg"),
                               flat_state(adam, params, "exp_avg"))
        finally:
            close_peer(peer)
            del broker

    @pytest.mark.timeout(120)
    def test_impala_env_switch_and_flag_off(self, monkeypatch):
        monkeypatch.setenv("MOOLIB_AMD_FUSED_OPT", "1")
        peer, broker = make_impala_peer("cpu", autocast_bf16=False, fused_optimizer=False)
        try:
            assert peer.cfg.fused_optimizer and isinstance(peer.optimizer, FlatAdam)
        finally:
            close_peer(peer)
            del broker
        monkeypatch.delenv("MOOLIB_AMD_FUSED_OPT")
        peer, broker = make_impala_peer("cpu", autocast_bf16=False, fused_optimizer=False)
        try:
            assert type(peer.optimizer) is torch.optim.Adam and peer.scheduler is not None
        finally:
            close_peer(peer)
            del broker


# =============================================================== GPU tests


def atari_shapes(use_lstm):
    from moolib_amd.models.atari import AtariNet

    torch.manual_seed(2)
    return [p.detach().clone() for p in AtariNet(num_actions=18, use_lstm=use_lstm).parameters()]


@gpu
@requires_gpu
class TestKernels:
    def test_constants(self):
        from moolib_amd import _kernels

        assert _kernels.FLAT_ADAM_PASS_ELEMENTS == ops.PASS_ELEMENTS
        assert _kernels.FLAT_ADAM_MAX_BLOCKS == ops.MAX_BLOCKS

    @pytest.mark.parametrize("N", KERNEL_N)
    def test_integer_exact(self, N):
        for kind in int_kinds(N):
            check_int_equal(run_int("cuda", N, kind), N, kind)

    def test_without_shadow(self):
        p, g, max_norm = R.integer_case(1025, "clip")
        z = torch.zeros(1025)
        out = run_op("cuda", p, g, z, z, 0, R.INT["lr"], R.INT["beta1"], R.INT["beta2"],
                     R.INT["eps"], max_norm, shadow=False)
        assert torch.equal(out["p"].double(), R.integer_ref(1025, "clip").p)

    @pytest.mark.parametrize("scale,eps,max_norm", FLOAT_CASES)
    def test_float(self, scale, eps, max_norm):
        p, g, m, v = R.float_case(FLOAT_N, scale, eps, max_norm)
        out = run_op("cuda", p, g, m, v, R.FLOAT_STEP, R.FLOAT["lr"], R.FLOAT["beta1"],
                     R.FLOAT["beta2"], eps, max_norm)
        _, e_ref = eager_float(FLOAT_N, scale, eps, max_norm)
        check_float(out, R.float_ref(FLOAT_N, scale, eps, max_norm), e_ref,
                    "kernel_float scale=%g eps=%g max_norm=%s" % (scale, eps, max_norm))
        assert int(out["step"]) == R.FLOAT_STEP + 1

    @pytest.mark.parametrize("max_norm", R.FLOAT_MAX_NORM)
    def test_float_two_passes(self, max_norm):
        N = P + 1
        p, g, m, v = R.float_case(N, 1.0, 1e-8, max_norm)
        out = run_op("cuda", p, g, m, v, R.FLOAT_STEP, R.FLOAT["lr"], R.FLOAT["beta1"],
                     R.FLOAT["beta2"], 1e-8, max_norm)
        _, e_ref = eager_float(N, 1.0, 1e-8, max_norm)
        check_float(out, R.float_ref(N, 1.0, 1e-8, max_norm), e_ref,
                    "kernel_float N=P+1 max_norm=%s" % max_norm)

    def test_nonfinite_gradient_propagates(self):
        p, g, m, v = (x.clone() for x in R.float_case(FLOAT_N, 1.0, 1e-8, 40.0))
        g[3] = float("inf")
        out = run_op("cuda", p, g, m, v, 3, 6e-4, 0.9, 0.999, 1e-8, 40.0)
        want = run_op("cpu", p, g, m, v, 3, 6e-4, 0.9, 0.999, 1e-8, 40.0)
        assert float(out["norm"]) == float("inf") and int(out["step"]) == 4
        assert torch.equal(torch.isnan(out["p"]), torch.isnan(want["p"]))
        assert torch.equal(torch.isnan(out["shadow"].float()), torch.isnan(want["shadow"].float()))
        assert bool(torch.isnan(out["p"][3]))

    def test_bit_reproducible(self):
        N = 2 ** 21 + 3
        p, g, m, v = R.float_case(N, 1.0, 1e-8, 40.0)
        args = (R.FLOAT_STEP, R.FLOAT["lr"], R.FLOAT["beta1"], R.FLOAT["beta2"], 1e-8, 40.0)
        a = run_op("cuda", p, g, m, v, *args)
        b = run_op("cuda", p, g, m, v, *args)
        for k in a:
            assert torch.equal(a[k], b[k]), k

    def test_kernel_rejects(self):
        from moolib_amd import _kernels

        z = lambda n=8, dt=torch.float32: torch.zeros(n, dtype=dt, device="cuda")
        ws = ops.new_workspace("cuda")
        step, lr = z(1, torch.int64), z(1)

        def call(p=None, g=None, shadow=None, step_next=None, partial=None, **kw):
            a = dict(beta1=0.9, beta2=0.999, eps=1e-8, max_norm=None)
            a.update(kw)
            _kernels.flat_adam_step(
                z() if p is None else p, z() if g is None else g, z(), z(), shadow, step,
                ws.step_next if step_next is None else step_next, lr,
                ws.partial if partial is None else partial, ws.norm,
                a["beta1"], a["beta2"], a["eps"], a["max_norm"])

        call()  # the baseline is accepted
        for kw in (dict(g=z(9)), dict(g=z(8, torch.float64)), dict(p=z(12)[1:9], g=z(8)),
                   dict(shadow=z(8)), dict(shadow=z(12, torch.bfloat16)[1:9]),
                   dict(step_next=step), dict(partial=z(8, torch.float64)),
                   dict(g=torch.zeros(8)), dict(beta1=1.0), dict(beta2=-0.1), dict(eps=-1.0),
                   dict(max_norm=0.0), dict(p=z(0), g=z(0))):
            with pytest.raises(RuntimeError, match="flat_adam_step"):
                call(**kw)
        torch.cuda.synchronize()

    def test_eager_switch(self, monkeypatch):
        monkeypatch.setenv("MOOLIB_AMD_NO_FUSED_OPT", "1")
        check_int_equal(run_int("cuda", 1025, "clip"), 1025, "clip")


def gpu_model_pair():
    a, b = make_models("cuda")
    return a, b, list(a.parameters()), list(b.parameters())


@gpu
@requires_gpu
class TestOptimizerGpu:
    def test_no_host_wait(self):
        model, _, params, _ = gpu_model_pair()
        opt = FlatAdam(params, max_grad_norm=CLIP, **HYPER)
        grads = [[g.cuda() for g in seeded_grads(params, 30 + s)] for s in range(3)]
        set_grads(params, grads[0])
        opt.step()  # kernels loaded, nothing left to allocate
        opt._step.zero_()
        torch.cuda.synchronize()
        mode = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for s in range(3):
                set_grads(params, grads[s])
                opt.param_groups[0]["lr"] = HYPER["lr"] * (0.5 ** s)
                norm = opt.step()
                opt.zero_grad()
        finally:
            torch.cuda.set_sync_debug_mode(mode)
        assert norm.is_cuda and int(opt._step) == 3
        assert float(opt._lr) == pytest.approx(HYPER["lr"] / 4, rel=1e-7)

    def test_capture_replays_bit_equal(self):
        """Three replays equal three eager steps bit for bit, step counter and
        lr included, starting from the same state."""
        from moolib_amd.parallel.graphs import GraphedCall

        _, _, pa, pb = gpu_model_pair()
        sa = [torch.nn.Parameter(p.detach().to(torch.bfloat16)) for p in pa]
        sb = [torch.nn.Parameter(p.detach().to(torch.bfloat16)) for p in pb]
        opt_a = FlatAdam(pa, max_grad_norm=CLIP, shadow_params=sa, **HYPER)
        opt_b = FlatAdam(pb, max_grad_norm=CLIP, shadow_params=sb, **HYPER)
        call = GraphedCall(lambda _i: opt_a.step(), warmup=1, name="flat_adam_test")
        g0 = [g.cuda() for g in seeded_grads(pa, 49)]
        set_grads(pa, g0)
        set_grads(pb, g0)
        call({})  # the warm-up call: an eager step
        call({})  # the capture (which executes nothing), then the first replay
        assert call.graph is not None and not call.failed
        opt_b.step()
        opt_b.step()
        for s in range(3):
            grads = [g.cuda() for g in seeded_grads(pa, 50 + s)]
            lr = HYPER["lr"] * (0.75 ** (s + 1))
            opt_a.param_groups[0]["lr"] = opt_b.param_groups[0]["lr"] = lr
            set_grads(pa, grads)
            set_grads(pb, grads)
            opt_a.sync_lr()
            na = call({}).clone()
            nb = opt_b.step().clone()
            assert torch.equal(na, nb)
            for name in ("_flat_p", "_m", "_v", "_step", "_lr"):
                assert torch.equal(getattr(opt_a, name), getattr(opt_b, name)), (name, s)
            assert torch.equal(opt_a._flat_shadow.view(torch.int16),
                               opt_b._flat_shadow.view(torch.int16))
        assert int(opt_a._step) == 5

    @pytest.mark.parametrize("use_lstm", [False, True], ids=["ff", "lstm"])
    def test_against_torch_on_device(self, use_lstm):
        """5 steps of FlatAdam and of clip_grad_norm_ + Adam(foreach=True) on
        AtariNet's parameter shapes: each within the float bound of the
        float64 reference at every step (not compared to each other)."""
        shapes = atari_shapes(use_lstm)
        max_norm = 40.0
        grads = [seeded_grads(shapes, 70 + s, scale=0.3) for s in range(5)]
        refs, errs = eager_trajectory(shapes, grads, max_norm=max_norm)
        assert refs[0].coef < 1.0, "the case must clip"
        pf = [torch.nn.Parameter(p.clone().cuda()) for p in shapes]
        pt = [torch.nn.Parameter(p.clone().cuda()) for p in shapes]
        fused = FlatAdam(pf, max_grad_norm=max_norm, **HYPER)
        adam = torch.optim.Adam(pt, foreach=True, **HYPER)
        worst = {"fused": 0.0, "torch": 0.0}
        for s in range(5):
            dev = [g.cuda() for g in grads[s]]
            set_grads(pf, dev)
            set_grads(pt, dev)
            nf = fused.step()
            nt = torch.nn.utils.clip_grad_norm_(pt, max_norm)
            adam.step()
            one = lambda x: torch.tensor([x], dtype=torch.float64)
            for name, params, opt, norm in (("fused", pf, fused, nf), ("torch", pt, adam, nt)):
                r = [
                    within(flat(params), refs[s].p, errs[s]["p"], (name, "p", s)),
                    within(flat_state(opt, params, "exp_avg"), refs[s].m, errs[s]["m"], (name, "m", s)),
                    within(flat_state(opt, params, "exp_avg_sq"), refs[s].v, errs[s]["v"], (name, "v", s)),
                    within(norm.reshape(1), one(refs[s].norm), errs[s]["norm"], (name, "norm", s)),
                ]
                worst[name] = max(worst[name], *r)
        _figure(test="atari_5_steps", use_lstm=use_lstm, N=int(flat(shapes).numel()),
                fused=round(worst["fused"], 4), torch=round(worst["torch"], 4))


@gpu
@requires_gpu
class TestLearnersGpu:
    def test_r2d2_learn(self):
        check_r2d2_learn("cuda")

    @pytest.mark.timeout(180)
    def test_impala_fused_step(self, monkeypatch):
        import test_rollout_integrity as RI
        from moolib_amd.parallel.graphs import GraphedCall

        monkeypatch.delenv("MOOLIB_AMD_FUSED_OPT", raising=False)
        peer, broker = make_impala_peer("cuda:0", grad_norm_clipping=1.0, learning_rate=3e-3)
        try:
            assert peer.bf16_shadow and isinstance(peer.optimizer, FlatAdam)
            assert peer.scheduler is not None and peer._graph_opt
            assert isinstance(peer._opt_call, GraphedCall)
            assert peer.optimizer._flat_p is peer._flat_master
            assert peer.optimizer._flat_shadow is peer._flat_shadow
            params = peer._master_params
            inp = RI._fixed_actor_input(peer.cfg.actor_batch_size, peer.cfg.device)
            peer.fwd_model.eval()
            f1, f2 = RI._fresh_outputs(peer, inp), RI._fresh_outputs(peer, inp)
            tol = 2.0 * RI._max_diff(f1, f2)

            def actor_sees_current_weights(before, what):
                fresh = RI._fresh_outputs(peer, inp)
                assert RI._max_diff(fresh, before) > tol, what + ": the weights did not move"
                for got in (RI._keep(peer._actor_call(inp)), RI._keep(peer._actor_fn(inp))):
                    if tol == 0.0:
                        assert all(torch.equal(got[k], fresh[k]) for k in fresh), what
                    else:
                        assert RI._max_diff(got, fresh) <= tol, what
                peer.fwd_model.eval()
                return fresh

            # an eager fused step (the graph's warm-up phase)
            ref, ratio = impala_ref_step(peer, params, 0, seed=21)
            assert ref.coef < 1.0, "the case must clip"
            assert torch.equal(peer._flat_shadow.view(torch.int16),
                               peer._flat_master.to(torch.bfloat16).view(torch.int16))
            fa = actor_sees_current_weights(f1, "after an eager fused step")
            # past the warm-up: capture, then replays, the scheduler moving lr
            steps = peer._opt_call.warmup + 3
            for s in range(1, steps):
                ref, r = impala_ref_step(peer, params, s, seed=21 + s)
                ratio = max(ratio, r)
            assert peer._opt_call.graph is not None and not peer._opt_call.failed
            assert int(peer.optimizer._step) == steps == peer.model_version
            assert torch.equal(peer._flat_shadow.view(torch.int16),
                               peer._flat_master.to(torch.bfloat16).view(torch.int16))
            actor_sees_current_weights(fa, "after graphed fused steps")
            _figure(test="impala_fused_step", steps=steps, p=round(ratio, 4))
        finally:
            close_peer(peer)
            del broker
