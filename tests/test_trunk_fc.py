"""trunk_fc (hip/fc.hip.inc) against an fp64 reference written from the formula,
the AtariNet route, the eager path and the host checks. docs/KERNEL_TESTS.md,
"Trunk FC", has the inputs, the bounds and the figures seen."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

import trunk_refs as TR

gpu = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")
BF16 = torch.bfloat16


def make_inputs(M, hw, integer, seed=0):
    """(x, W, b, dY): small integers with a sparse W, or bf16-exact floats."""
    g = torch.Generator().manual_seed(seed)
    K = 32 * hw[0] * hw[1]
    if integer:
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).double()  # noqa: E731
        W = ri(-1, 1, 256, K) * (torch.rand(256, K, generator=g) < 0.375)  # 3/4 zeros
        return ri(-2, 2, M, 32, *hw), W, ri(-3, 3, 256), ri(-3, 3, M, 256)
    r = lambda sd, *s: (sd * torch.randn(*s, generator=g)).to(BF16).double()  # noqa: E731
    return r(1, M, 32, *hw), r(0.02, 256, K), r(0.1, 256), r(1, M, 256)


def reference(x, W, b, dY, relu_in, mask=None):
    """fp64 value and n*S of every output: {name: (ref, n*S)}. `mask` replaces
    the reference's own pre > 0."""
    M, K = x.shape[0], W.shape[1]
    a = (x.relu() if relu_in else x).reshape(M, K)  # the NCHW flatten
    pre = a @ W.T + b
    dZ = dY * (pre > 0 if mask is None else mask)
    dx, dx_nS = dZ @ W, 256 * (dZ.abs() @ W.abs())
    if relu_in:
        dx, dx_nS = dx * (x.reshape(M, K) > 0), dx_nS * (x.reshape(M, K) > 0)
    return {
        "pre": (pre, (K + 1) * (a.abs() @ W.abs().T + b.abs())),
        "dx": (dx.reshape(x.shape), dx_nS.reshape(x.shape)),
        "dW": (dZ.T @ a, M * (dZ.abs().T @ a.abs())),
        "db": (dZ.sum(0), M * dZ.abs().sum(0)),
    }


def run_op(x, W, b, dY, relu_in, wdtype=torch.float32, split_k=None, nchw=False):
    from moolib_amd.ops.fc import trunk_fc

    x = x.to(BF16).cuda()
    if not nchw:
        x = x.contiguous(memory_format=torch.channels_last)
    x.requires_grad_()
    W, b = (t.to(wdtype).cuda().requires_grad_() for t in (W, b))
    feat = trunk_fc(x, W, b, relu_in=relu_in, split_k=split_k)
    feat.backward(dY.to(BF16).cuda())
    assert feat.dtype == x.grad.dtype == BF16 and feat.shape == dY.shape
    assert x.grad.shape == x.shape
    assert nchw or x.grad.is_contiguous(memory_format=torch.channels_last)
    return {"feat": feat.detach().cpu(), "dx": x.grad.cpu(), "dW": W.grad.cpu(), "db": b.grad.cpu()}


# M: 1; a 32-row forward tile + 1; two 512-row wgrad slabs + 1 (64-row forward
# tiles). Pixels: 1; 3x3 and 5x5 (no multiple of the 8-pixel chunk); 11x11.
# split_k: single pass, two slabs, the (M, P) rule, above P (clamped to P).
@gpu
@requires_gpu
@pytest.mark.parametrize("M,hw,relu_in,wdtype,split_k", [
    (1, (1, 1), True, torch.float32, None), (1, (11, 11), False, BF16, 2),
    (33, (3, 3), True, BF16, 100), (33, (11, 11), True, torch.float32, None),
    (33, (5, 5), False, torch.float32, 2), (130, (11, 11), True, torch.float32, 1),
    (130, (11, 11), False, BF16, None), (1025, (1, 1), False, BF16, 1),
    (1025, (5, 5), True, BF16, None), (1025, (11, 11), True, torch.float32, None),
    (1025, (11, 11), False, torch.float32, 2),
])
def test_integer_exact(M, hw, relu_in, wdtype, split_k):
    x, W, b, dY = make_inputs(M, hw, integer=True)
    ref = {k: v[0] for k, v in reference(x, W, b, dY, relu_in).items()}
    assert ref["pre"].abs().max() <= 256 and ref["dx"].abs().max() <= 256  # bf16 holds them
    got = run_op(x, W, b, dY, relu_in, wdtype, split_k, nchw=(M == 33))
    assert torch.equal(got["feat"].double(), ref["pre"].relu())
    assert torch.equal(got["dx"].double(), ref["dx"])
    for k in ("dW", "db"):  # exact in fp32; autograd rounds them once for bf16 parameters
        assert got[k].dtype == wdtype and torch.equal(got[k], ref[k].to(wdtype)), k
    if relu_in:
        assert not got["dx"][x <= 0].any()


@gpu
@requires_gpu
def test_random_float():
    """Per element 2^-8 |ref| for the bf16 outputs plus 2^-23 n S; the
    reference's backward takes feat > 0 from the op's own forward."""
    x, W, b, dY = make_inputs(130, (11, 11), integer=False)
    got = run_op(x, W, b, dY, True)
    ref = reference(x, W, b, dY, True, mask=got["feat"] > 0)
    ref["feat"] = (ref["pre"][0].relu(), ref.pop("pre")[1])
    assert set(ref) == set(got)
    for k, (want, nS) in ref.items():
        rel = 2.0**-8 if got[k].dtype == BF16 else 0.0
        err = (got[k].double() - want).abs()
        over = err - (rel * want.abs() + 2.0**-23 * nS)
        print(k, "max err %.3e, worst err/bound %.3f"
              % (err.max(), (err / (rel * want.abs() + 2.0**-23 * nS).clamp_min(1e-300)).max()))
        assert (over <= 0).all(), k


@gpu
@requires_gpu
def test_deterministic():
    inputs = make_inputs(1025, (11, 11), integer=False)
    a, b = run_op(*inputs, True), run_op(*inputs, True)
    assert all(torch.equal(a[k], b[k]) for k in a)


@gpu
@requires_gpu
@pytest.mark.parametrize("mode", ["a", "b"])
def test_model_route(mode, monkeypatch):
    """(a) bf16 shadow weights, (b) fp32 weights under autocast. The fused
    route's outputs within test_trunk_composed's derived bound of R_exact:
    2 d + 2^-8 max|R_exact|, d = max|R_emul - R_exact|."""
    from moolib_amd.models.atari import AtariNet
    from moolib_amd.ops import fc as fc_ops

    params, inputs, core, grads = TR.float_case(False)
    ex = TR.exact(params, inputs, core, grads)
    em = TR.atari_ref(params, inputs, core, mode, "wrw", grads)
    model = AtariNet(num_actions=6, fused_trunk_fc=True)
    model.load_state_dict({k: v.float() for k, v in params.items()})
    model = model.cuda()
    if mode == "a":
        model = model.to(BF16).to(memory_format=torch.channels_last)
    inputs = {k: v.cuda() for k, v in inputs.items()}
    calls = []
    op = fc_ops.trunk_fc
    monkeypatch.setattr(fc_ops, "trunk_fc", lambda *a, **k: calls.append(1) or op(*a, **k))
    amp = (lambda: torch.autocast("cuda", dtype=BF16)) if mode == "b" else contextlib.nullcontext
    outs = {}
    for fused in (False, True):
        model.fused_trunk_fc = fused
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
        assert TR.float_within(outs[True][k].detach().cpu(), ex[k], bound), k
    out = outs[True]
    ((out["policy_logits"] * grads["policy_logits"].cuda()).sum()
     + (out["baseline"] * grads["baseline"].cuda()).sum()).backward()
    for k, p in model.named_parameters():
        assert p.grad is not None and p.grad.isfinite().all() and p.grad.any(), k


@gpu
@requires_gpu
@pytest.mark.parametrize("case", ["16 channels", "weight shape", "weight not contiguous", "x fp32"])
def test_host_rejections(case):
    from moolib_amd.ops.fc import trunk_fc

    C = 16 if case == "16 channels" else 32
    x = torch.zeros(4, C, 3, 3, device="cuda", dtype=torch.float32 if case == "x fp32" else BF16)
    W = torch.zeros(256, C * 9 + (1 if case == "weight shape" else 0), device="cuda")
    if case == "weight not contiguous":
        W = torch.zeros(C * 9, 256, device="cuda").t()
    with pytest.raises(ValueError):
        trunk_fc(x, W, torch.zeros(256, device="cuda"))


@pytest.mark.parametrize("relu_in", [False, True])
@pytest.mark.parametrize("channels_last", [False, True])
def test_eager_is_linear_on_the_nchw_flatten(relu_in, channels_last):
    from moolib_amd.ops.fc import trunk_fc, trunk_fc_eager

    g = torch.Generator().manual_seed(1)
    x = torch.randn(5, 32, 3, 2, generator=g, dtype=torch.float64)
    W = torch.randn(256, 192, generator=g, dtype=torch.float64)
    b = torch.randn(256, generator=g, dtype=torch.float64)
    want = F.relu(F.linear((x.relu() if relu_in else x).flatten(1), W, b))
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    for op in (trunk_fc_eager, trunk_fc):  # on the CPU trunk_fc is the eager path
        got = op(x, W, b, relu_in)
        assert got.dtype == torch.float64 and (got - want).abs().max() <= 1e-12


def test_interface():
    from moolib_amd.impala import ImpalaConfig
    from moolib_amd.models.atari import AtariNet, create_model
    from moolib_amd.ops.fc import trunk_fc_available

    shapes = lambda m: [(k, tuple(v.shape)) for k, v in m.state_dict().items()]  # noqa: E731
    default = AtariNet(num_actions=6)
    assert shapes(AtariNet(num_actions=6, fused_trunk_fc=True)) == shapes(default)
    assert create_model(num_actions=6, fused_trunk_fc=True).fused_trunk_fc
    assert not default.fused_trunk_fc and not create_model(num_actions=6).fused_trunk_fc
    assert ImpalaConfig().fused_trunk_fc is False
    assert not trunk_fc_available(32, torch.device("cpu"))
    assert not trunk_fc_available(16, torch.device("cuda"))
