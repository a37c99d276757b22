"""policy_value_heads (hip/heads.hip.inc) against an fp64 reference written from
the formulas, the AtariNet route, the eager path and the host checks.
docs/KERNEL_TESTS.md, "Policy and baseline heads", has the inputs, the bounds
and the figures seen."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

import trunk_refs as TR

gpu = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")
BF16 = torch.bfloat16
F32 = torch.float32
PARAMS = ("Wp", "bp", "Wb", "bb")


def make_inputs(M, A, D, composite, integer, seed=0):
    """fp64 x, Wp, bp, Wb, bb, reward, action, dL, dB: small integers with a
    sparse weight, or bf16-exact floats (the reward is fp32 in both)."""
    g = torch.Generator().manual_seed(seed)
    K = D + 1 + A if composite else D
    shapes = {"x": (M, D), "Wp": (A, K), "bp": (A,), "Wb": (1, K), "bb": (1,), "dL": (M, A),
              "dB": (M,)}
    if integer:
        t = {k: torch.randint(-2, 3, s, generator=g).double() for k, s in shapes.items()}
        for k in ("Wp", "Wb"):  # 5/8 zeros, the rest +-1
            t[k] = t[k].sign() * (torch.rand(t[k].shape, generator=g) < 0.625)
        t["reward"] = torch.randint(-4, 5, (M,), generator=g).double() / 2
        t["action"] = torch.randint(-1, A + 2, (M,), generator=g)  # -1, A, A+1: out of range
    else:
        sd = {"Wp": 0.05, "Wb": 0.05, "bp": 0.1, "bb": 0.1}
        t = {k: (sd.get(k, 1.0) * torch.randn(s, generator=g)).to(BF16).double()
             for k, s in shapes.items()}
        t["reward"] = (1.5 * torch.randn(M, generator=g)).double()
        t["action"] = torch.randint(0, A, (M,), generator=g)
    if not composite:
        t["reward"] = t["action"] = None
    return t


def reference(t, with_dB=True):
    """fp64 value and n*S of every output: {name: (ref, n*S)}."""
    A, D = t["Wp"].shape[0], t["x"].shape[1]
    Z = t["x"]
    if t["reward"] is not None:
        a = t["action"]
        onehot = F.one_hot(a.clamp(0, A - 1), A).double() * ((a >= 0) & (a < A)).unsqueeze(1)
        Z = torch.cat([Z, t["reward"].clamp(-1, 1).unsqueeze(1), onehot], dim=1)
    W, b = torch.cat([t["Wp"], t["Wb"]]), torch.cat([t["bp"], t["bb"]])
    dOut = torch.cat([t["dL"], (t["dB"] if with_dB else 0 * t["dB"]).unsqueeze(1)], dim=1)
    M, K = Z.shape
    out, out_nS = Z @ W.T + b, (K + 1) * (Z.abs() @ W.abs().T + b.abs())
    dW, dW_nS = dOut.T @ Z, M * (dOut.abs().T @ Z.abs())
    db, db_nS = dOut.sum(0), M * dOut.abs().sum(0)
    return {
        "logits": (out[:, :A], out_nS[:, :A]), "baseline": (out[:, A], out_nS[:, A]),
        "dx": ((dOut @ W)[:, :D], (A + 1) * (dOut.abs() @ W.abs())[:, :D]),
        "Wp": (dW[:A], dW_nS[:A]), "Wb": (dW[A:], dW_nS[A:]),
        "bp": (db[:A], db_nS[:A]), "bb": (db[A:], db_nS[A:]),
    }


def run_op(t, wdtype=F32, with_dB=True):
    from moolib_amd.ops.heads import policy_value_heads

    x = t["x"].to(BF16).cuda().requires_grad_()
    p = {k: t[k].to(wdtype).cuda().requires_grad_() for k in PARAMS}
    extra = () if t["reward"] is None else (t["reward"].float().cuda(), t["action"].cuda())
    logits, baseline = policy_value_heads(x, *(p[k] for k in PARAMS), *extra)
    assert logits.dtype == baseline.dtype == F32
    assert logits.shape == t["dL"].shape and baseline.shape == t["dB"].shape
    outs, grads = [logits], [t["dL"].float().cuda()]
    if with_dB:
        outs, grads = outs + [baseline], grads + [t["dB"].float().cuda()]
    torch.autograd.backward(outs, grads)
    assert x.grad.dtype == BF16 and all(p[k].grad.dtype == wdtype for k in PARAMS)
    got = {"logits": logits, "baseline": baseline, "dx": x.grad}
    got.update({k: p[k].grad for k in PARAMS})
    return {k: v.detach().cpu() for k, v in got.items()}


# M: 1; a 16-row forward tile + 1; one 128-row backward slab + 1; two slabs + 1;
# 64-row forward tiles (from 1024 rows) + 1. A: N = A + 1 = 16 exactly (15),
# crossing a tile (16, 18), the maximum (63). The last flag drops dbaseline.
@gpu
@requires_gpu
@pytest.mark.parametrize("M,A,D,composite,wdtype,with_dB", [
    (1, 1, 128, False, F32, True), (1, 63, 512, False, F32, True),
    (17, 15, 256, False, BF16, True), (17, 18, 256, True, F32, True),
    (129, 16, 512, False, F32, True), (129, 63, 256, True, BF16, True),
    (257, 18, 256, True, F32, False), (257, 63, 512, False, BF16, True),
    (257, 15, 256, True, BF16, True), (1025, 18, 256, True, F32, True),
    (1025, 16, 128, False, BF16, True), (1025, 1, 256, True, F32, True),
])
def test_integer_exact(M, A, D, composite, wdtype, with_dB):
    t = make_inputs(M, A, D, composite, integer=True)
    ref = {k: v[0] for k, v in reference(t, with_dB).items()}
    assert ref["dx"].abs().max() <= 256  # bf16 holds it
    got = run_op(t, wdtype, with_dB)
    assert set(got) == set(ref)
    for k in got:  # parameter gradients: exact in fp32, rounded once for bf16 parameters
        want = ref[k].to(wdtype) if k in PARAMS else ref[k]
        assert torch.equal(got[k].double(), want.double()), k


@gpu
@requires_gpu
@pytest.mark.parametrize("A,D,composite", [(18, 256, True), (18, 512, False)])
def test_random_float(A, D, composite):
    """Per element 2^-8 |ref| for the bf16 output (d_x) plus 2^-23 n S."""
    t = make_inputs(257, A, D, composite, integer=False)
    got, ref = run_op(t), reference(t)
    for k, (want, nS) in ref.items():
        bound = (2.0**-8 if got[k].dtype == BF16 else 0.0) * want.abs() + 2.0**-23 * nS
        err = (got[k].double() - want).abs()
        print(k, "max err %.3e, worst err/bound %.3f"
              % (err.max(), (err / bound.clamp_min(1e-300)).max()))
        assert (err <= bound).all(), k


@gpu
@requires_gpu
@pytest.mark.parametrize("D,composite", [(256, True), (512, False)])
def test_deterministic(D, composite):
    t = make_inputs(257, 18, D, composite, integer=False)
    a, b = run_op(t), run_op(t)
    assert all(torch.equal(a[k], b[k]) for k in a)


@gpu
@requires_gpu
@pytest.mark.parametrize("mode", ["a", "b"])
def test_model_route(mode, monkeypatch):
    """(a) bf16 shadow weights, (b) fp32 weights under autocast, no LSTM: the
    fused route's outputs within 2 d + 2^-8 max|R_exact| of R_exact."""
    from moolib_amd.models.atari import AtariNet
    from moolib_amd.ops import heads as heads_ops

    params, inputs, core, grads = TR.float_case(False)
    ex = TR.exact(params, inputs, core, grads)
    em = TR.atari_ref(params, inputs, core, mode, "wrw", grads)
    model = AtariNet(num_actions=6, fused_heads=True)
    model.load_state_dict({k: v.float() for k, v in params.items()})
    model = model.cuda()
    if mode == "a":
        model = model.to(BF16).to(memory_format=torch.channels_last)
    inputs = {k: v.cuda() for k, v in inputs.items()}
    calls = []
    op = heads_ops.policy_value_heads
    monkeypatch.setattr(heads_ops, "policy_value_heads",
                        lambda *a, **k: calls.append(1) or op(*a, **k))
    amp = (lambda: torch.autocast("cuda", dtype=BF16)) if mode == "b" else contextlib.nullcontext
    outs = {}
    for fused in (False, True):
        model.fused_heads = fused
        with amp():
            outs[fused], _ = model(inputs, tuple())
        assert len(calls) == int(fused)
    with amp(), torch.no_grad():
        model(inputs, tuple())
    assert len(calls) == 2
    for k in ("policy_logits", "baseline"):
        _, bound = TR.float_bound(ex[k], em[k])
        err = {f: (outs[f][k].detach().cpu().double() - ex[k]).abs().max().item() for f in outs}
        print(mode, k, "err default %.3e fused %.3e bound %.3e" % (err[False], err[True], bound))
        assert outs[True][k].dtype == F32 and TR.float_within(outs[True][k].detach().cpu(), ex[k], bound), k
    out = outs[True]
    ((out["policy_logits"] * grads["policy_logits"].cuda()).sum()
     + (out["baseline"] * grads["baseline"].cuda()).sum()).backward()
    for k, p in model.named_parameters():
        assert p.grad is not None and p.grad.isfinite().all() and p.grad.any(), k


@gpu
@requires_gpu
def test_model_route_lstm():
    """lstm_size=512: on the same core_output the fused heads are at least as
    close to the fp64 heads as the default route's bf16 GEMMs."""
    from moolib_amd.models.atari import AtariNet

    params, inputs, core, _ = TR.core_float_case(512)
    model = AtariNet(num_actions=6, use_lstm=True, lstm_size=512)
    model.load_state_dict({k: v.float() for k, v in params.items()})
    model = model.cuda().to(BF16).to(memory_format=torch.channels_last)
    inputs = {k: v.cuda() for k, v in inputs.items()}
    seen, outs = [], {}
    model.policy.register_forward_pre_hook(lambda m, a: seen.append(a[0].detach()))
    for fused in (False, True):
        model.fused_heads = fused
        with torch.no_grad():
            outs[fused], _ = model(inputs, tuple(s.cuda() for s in core))
    assert len(seen) == 1 and seen[0].dtype == BF16  # the fused route never calls self.policy
    h = seen[0].double()
    want = {"policy_logits": h @ model.policy.weight.double().T + model.policy.bias.double(),
            "baseline": (h @ model.baseline.weight.double().T + model.baseline.bias.double())[:, 0]}
    for k, w in want.items():
        err = {f: (outs[f][k].double().reshape(w.shape) - w).abs().max().item() for f in outs}
        print(k, "err default %.3e fused %.3e" % (err[False], err[True]))
        assert err[True] <= err[False], k


@gpu
@requires_gpu
@pytest.mark.parametrize("case", ["D = 384", "A = 64", "weight not contiguous", "x fp32",
                                  "reward without prev_action"])
def test_host_rejections(case):
    from moolib_amd.ops.heads import policy_value_heads

    D = 384 if case == "D = 384" else 256
    A = 64 if case == "A = 64" else 6
    z = lambda *s, **k: torch.zeros(*s, device="cuda", **k)  # noqa: E731
    x = z(4, D, dtype=F32 if case == "x fp32" else BF16)
    Wp = z(D, A).t() if case == "weight not contiguous" else z(A, D)
    kw = {"reward": z(4)} if case == "reward without prev_action" else {}
    with pytest.raises(ValueError):
        policy_value_heads(x, Wp, z(A), z(1, D), z(1), **kw)


@pytest.mark.parametrize("composite", [False, True])
def test_cpu_is_eager(composite):
    from moolib_amd.ops.heads import heads_eager, policy_value_heads

    t = make_inputs(5, 6, 256, composite, integer=False, seed=1)
    args = [t[k].float() for k in ("x",) + PARAMS]
    x = args[0]
    if composite:
        t["action"][0] = 2
        args += [t["reward"].float(), t["action"]]
        x = torch.cat([x, args[5].view(-1, 1).clamp(-1, 1), F.one_hot(t["action"], 6).float()], -1)
    want = (F.linear(x, args[1], args[2]).float(), F.linear(x, args[3], args[4]).float().view(-1))
    for op in (heads_eager, policy_value_heads):  # on the CPU the op is the eager path
        got = op(*args)
        assert all(torch.equal(g, w) for g, w in zip(got, want))


def test_interface():
    from moolib_amd.impala import ImpalaConfig
    from moolib_amd.models.atari import AtariNet, create_model
    from moolib_amd.ops.heads import heads_available

    shapes = lambda m: [(k, tuple(v.shape)) for k, v in m.state_dict().items()]  # noqa: E731
    default, fused = AtariNet(num_actions=6), AtariNet(num_actions=6, fused_heads=True)
    assert shapes(fused) == shapes(default)
    assert create_model(num_actions=6, fused_heads=True).fused_heads
    assert not default.fused_heads and not create_model(num_actions=6).fused_heads
    assert ImpalaConfig().fused_heads is False
    assert not heads_available(256, 6, True, torch.device("cpu"))
    assert not heads_available(256, 64, False, torch.device("cuda"))
    fused.load_state_dict(default.state_dict())
    _, inputs, _, _ = TR.float_case(False, T=1, B=2)
    with torch.no_grad():
        torch.manual_seed(0)
        a, _ = default(inputs, tuple())
        torch.manual_seed(0)
        b, _ = fused(inputs, tuple())
    assert all(torch.equal(a[k], b[k]) for k in a)
