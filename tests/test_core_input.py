"""core_input_projection (hip/lstm_input.hip.inc) against an fp64 reference, the
AtariNet route, the eager path and the host checks. feat, the weight and the
upstream gradient are bf16-exact, so the reference and the kernels see the same
numbers and the bounds are those of docs/KERNEL_TESTS.md: one bf16 rounding plus
fp32 accumulation of n terms whose absolute values sum to S."""
import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")
BF16 = torch.bfloat16


def make_inputs(M, A, H, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    feat = r(M, 256).relu().to(BF16)
    reward = 2 * r(M)
    fixed = torch.tensor([1.0, -1.0, 3.0, -2.5])[:M]
    reward[: len(fixed)] = fixed  # exactly +-1 and outside +-1
    # action 1 is never taken when there are three or more; 0 and A-1 are
    taken = torch.tensor([a for a in range(A) if a != 1 or A < 3])
    action = taken[torch.randint(len(taken), (M,), generator=g)]
    action[0], action[-1] = 0, (A - 1 if M > 1 else 0)
    W = (0.1 * r(4 * H, 257 + A)).to(BF16)
    return feat, reward, action, W, 0.1 * r(4 * H), 0.1 * r(4 * H), r(M, 4 * H).to(BF16)


def reference(feat, reward, action, W, b_ih, b_hh, G):
    """fp64 value and n*S of every output: {name: (ref, n*S)}."""
    A = W.shape[1] - 257
    f, W, G, b_ih, b_hh = (t.double() for t in (feat, W, G, b_ih, b_hh))
    valid = ((action >= 0) & (action < A)).unsqueeze(1)
    onehot = F.one_hot(action.clamp(0, A - 1), A).double() * valid
    Z = torch.cat([f, reward.double().clamp(-1, 1).unsqueeze(1), onehot], 1)
    M, N = G.shape
    return {
        "Xg": (Z @ W.T + b_ih + b_hh, 260 * (Z.abs() @ W.abs().T + b_ih.abs() + b_hh.abs())),
        "d_feat": (G @ W[:, :256], N * (G.abs() @ W[:, :256].abs())),
        "dW": (G.T @ Z, M * (G.abs().T @ Z.abs())),
        "db": (G.sum(0), M * G.abs().sum(0)),
    }


def run_op(feat, reward, action, W, b_ih, b_hh, G, wdtype=torch.float32):
    from moolib_amd.ops.lstm import core_input_projection

    feat = feat.cuda().requires_grad_()
    W, b_ih, b_hh = (t.to(wdtype).cuda().requires_grad_() for t in (W, b_ih, b_hh))
    Xg = core_input_projection(feat, reward.cuda(), action.cuda(), W, b_ih, b_hh)
    Xg.backward(G.cuda())
    assert Xg.dtype == feat.grad.dtype == BF16 and Xg.shape == G.shape
    assert torch.equal(b_ih.grad, b_hh.grad)
    return {"Xg": Xg.detach(), "d_feat": feat.grad, "dW": W.grad, "db": b_ih.grad}


def check(got, ref):
    for k, (want, nS) in ref.items():
        rel = 2.0**-8 if got[k].dtype == BF16 else 0.0
        err = (got[k].cpu().double() - want).abs()
        over = err - (rel * want.abs() + 2.0**-23 * nS)
        print(k, "max err %.3e, worst err - bound %.3e" % (err.max(), over.max()))
        assert (over <= 0).all(), k


# M: 1; a 32-row forward tile + 1; two 512-row wgrad slabs + 1 (64-row forward tiles)
@gpu
@requires_gpu
@pytest.mark.parametrize("M,A,H,wdtype", [
    (1, 18, 128, torch.float32), (33, 1, 128, BF16), (33, 62, 512, torch.float32),
    (100, 6, 256, torch.float32), (1025, 18, 128, BF16), (1025, 62, 512, torch.float32),
    (1025, 1, 512, BF16),
])
def test_forward_backward_fp64(M, A, H, wdtype):
    inputs = make_inputs(M, A, H)
    # bf16 biases are the bf16 model's; the reference sees what the kernel sees
    if wdtype == BF16:
        inputs = inputs[:4] + tuple(b.to(BF16).float() for b in inputs[4:6]) + inputs[6:]
    got = run_op(*inputs, wdtype=wdtype)
    # autograd rounds the fp32 dW and db to bf16 for bf16 parameters: check()
    # then allows them the one bf16 rounding, as it does for Xg and d_feat
    check(got, reference(*inputs))
    if A >= 3:
        assert not got["dW"][:, 257 + 1].any()  # the action never taken


@gpu
@requires_gpu
def test_out_of_range_actions():
    feat, reward, _, W, b_ih, b_hh, G = make_inputs(8, 6, 128)
    action = torch.tensor([-1, 6, 2**40, -(2**40), 255, -1, 6, 7])
    got = run_op(feat, reward, action, W, b_ih, b_hh, G)
    check(got, reference(feat, reward, action, W, b_ih, b_hh, G))
    assert not got["dW"][:, 257:].any()
    narrow = run_op(feat, reward, action.clamp(-1, 255).to(torch.int16), W, b_ih, b_hh, G)
    assert all(torch.equal(got[k], narrow[k]) for k in got)


@gpu
@requires_gpu
def test_backward_is_deterministic():
    inputs = make_inputs(1025, 18, 128)
    a, b = run_op(*inputs), run_op(*inputs)
    assert all(torch.equal(a[k], b[k]) for k in a)


@gpu
@requires_gpu
def test_model_route(monkeypatch):
    # a route check; what the route computes (outputs, state, every gradient)
    # is held to float64 in tests/test_core_composed.py
    from moolib_amd.models.atari import AtariNet
    from moolib_amd.ops import lstm as lstm_ops

    torch.manual_seed(7)
    model = AtariNet(num_actions=6, use_lstm=True, lstm_size=512, fused_core_input=True)
    model = model.to("cuda").to(BF16)
    T, B = 3, 2
    done = torch.zeros(T, B, dtype=torch.bool, device="cuda")
    done[1, 0] = True
    inputs = {
        "state": torch.randint(0, 256, (T, B, 4, 84, 84), dtype=torch.uint8, device="cuda"),
        "reward": 2 * torch.randn(T, B, device="cuda"),
        "done": done,
        "prev_action": torch.randint(0, 6, (T, B), device="cuda"),
    }
    core = tuple(t.cuda().to(BF16) for t in model.initial_state(batch_size=B))
    calls = []
    op = lstm_ops.core_input_projection
    monkeypatch.setattr(lstm_ops, "core_input_projection", lambda *a: calls.append(1) or op(*a))
    with torch.no_grad():
        fused, _ = model(inputs, core)
        assert len(calls) == 1
        model.fused_core_input = False
        plain, _ = model(inputs, core)
        assert len(calls) == 1
    diff = (fused["policy_logits"] - plain["policy_logits"]).abs().max().item()
    assert diff <= 0.15, diff

    model.fused_core_input = True
    out, _ = model(inputs, core)
    assert len(calls) == 2
    (out["policy_logits"].sum() + out["baseline"].sum()).backward()
    for p in (model.core.weight_ih_l0, model.core.bias_ih_l0, model.core.bias_hh_l0,
              model.fc.weight):
        assert p.grad is not None and p.grad.isfinite().all() and p.grad.any()


def test_eager_path_is_the_formula():
    from moolib_amd.ops.lstm import core_input_projection

    feat, reward, action, W, b_ih, b_hh, _ = (t.double() if t.is_floating_point() else t
                                              for t in make_inputs(9, 5, 16))
    x = torch.cat([feat, reward.clamp(-1, 1).unsqueeze(1), F.one_hot(action, 5).double()], 1)
    got = core_input_projection(feat, reward, action, W, b_ih, b_hh)
    assert got.dtype == torch.float64
    assert (got - F.linear(x, W, b_ih + b_hh)).abs().max() <= 1e-12


def test_interface():
    from moolib_amd.models.atari import AtariNet, create_model
    from moolib_amd.ops import lstm as lstm_ops

    shapes = lambda m: [(k, tuple(v.shape)) for k, v in m.state_dict().items()]  # noqa: E731
    default = AtariNet(num_actions=6, use_lstm=True)
    assert shapes(AtariNet(num_actions=6, use_lstm=True, fused_core_input=True)) == shapes(default)
    assert create_model(num_actions=6, use_lstm=True, fused_core_input=True).fused_core_input
    assert not default.fused_core_input
    cpu, cuda = torch.device("cpu"), torch.device("cuda")
    assert lstm_ops.CORE_INPUT_MAX_ACTIONS == 62
    assert not lstm_ops.core_input_available(256, 6, 256, cpu)
    assert not lstm_ops.core_input_available(256, 63, 256, cuda)
    assert not lstm_ops.core_input_available(256, 6, 64, cuda)


@gpu
@requires_gpu
@pytest.mark.parametrize("case", ["width 128", "63 actions", "bias length", "feat fp32",
                                  "weight not contiguous"])
def test_host_rejections(case):
    from moolib_amd.ops.lstm import core_input_projection

    width, A = (128 if case == "width 128" else 256), (63 if case == "63 actions" else 6)
    feat = torch.zeros(4, width, device="cuda", dtype=BF16)
    if case == "feat fp32":
        feat = feat.float()
    reward, action = torch.zeros(4, device="cuda"), torch.zeros(4, device="cuda", dtype=torch.int64)
    W = torch.zeros(512, width + 1 + A, device="cuda")
    if case == "weight not contiguous":
        W = torch.zeros(width + 1 + A, 512, device="cuda").t()
    bias = torch.zeros(256 if case == "bias length" else 512, device="cuda")
    with pytest.raises((ValueError, RuntimeError)):
        core_input_projection(feat, reward, action, W, bias, bias)
