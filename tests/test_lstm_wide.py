"""The LSTM scan for hidden sizes 128 and 512 (hip/lstm_wide.hip.inc) against
the fp64 references of tests/kernel_refs.py, its forward-only variant, the
AtariNet route and the host checks. docs/KERNEL_TESTS.md has the bound."""
import functools
import os

import pytest
import torch

import kernel_refs as R

gpu = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

BF16 = torch.bfloat16
SIZES = [128, 512]
# one step with one row; a 32-row tile plus one row; a 16-row tile plus one row
CASES = [(1, 1), (3, 33), (4, 17)]
# (absolute, fraction of max|reference|): LSTM_PRESENT of tests/test_kernel_edges.py
PRESENT = {"H": (3e-2, 0.0), "hT": (3e-2, 0.0), "cT": (3e-2, 0.0), "dX": (5e-2, 0.05),
           "dh0": (1e-1, 0.05), "dc0": (1e-1, 0.05), "dW": (2.0, 0.05)}


@functools.lru_cache(maxsize=None)
def refs(hidden, T, B):
    """(inputs, R_exact, R_emul), computed once per case and shared."""
    d = R.lstm_inputs(torch.Generator().manual_seed(hidden + 100 * T + B), T, B, hidden=hidden)
    return d, R.lstm_exact(d), R.lstm_emul(d)


def device_inputs(d, grad):
    X, h0 = (d[k].to(BF16).cuda().requires_grad_(grad) for k in ("X", "h0"))
    c0, w = (d[k].float().cuda().requires_grad_(grad) for k in ("c0", "w"))
    return X, d["nd"].float().cuda(), h0, c0, w


@gpu
@requires_gpu
@pytest.mark.parametrize("T,B", CASES)
@pytest.mark.parametrize("hidden", SIZES)
def test_forward_backward_fp64(hidden, T, B):
    """max|kernel - R_exact| <= min(2*d + 2**-8 * max|R_exact|, atol + rel * max|R_exact|)
    per tensor, d = max|R_emul - R_exact| from the CPU alone. At (1, 1) the only
    row is reset at t=0: dh0, dc0 and dW must be exact zeros."""
    from moolib_amd.ops.lstm import fused_lstm_scan

    d, exact, emul = refs(hidden, T, B)
    X, nd, h0, c0, w = device_inputs(d, True)
    H, hT, cT = fused_lstm_scan(X, nd, h0, c0, w)
    loss = ((H.float() * d["gH"].float().cuda()).sum()
            + (hT.float() * d["ghT"].float().cuda()).sum()
            + (cT * d["gcT"].float().cuda()).sum())
    loss.backward()
    got = {"H": H, "hT": hT, "cT": cT, "dX": X.grad, "dh0": h0.grad, "dc0": c0.grad,
           "dW": w.grad}
    failures = []
    for k, (dist, bound) in R.lstm_bounds(exact, emul).items():
        err = (got[k].detach().cpu().double() - exact[k]).abs().max().item()
        atol, rel = PRESENT[k]
        bound = min(bound, atol + rel * exact[k].abs().max().item())
        print("LSTM_WIDE_FIGURE", hidden, T, B, k, "d=%.3g err=%.3g bound=%.3g" % (dist, err, bound))
        if not err <= bound:
            failures.append((k, err, bound))
    assert not failures, failures


@gpu
@requires_gpu
@pytest.mark.parametrize("T,B", CASES)
@pytest.mark.parametrize("hidden", SIZES)
def test_forward_only_equals_saving_forward(hidden, T, B):
    from moolib_amd import _kernels
    from moolib_amd.ops.lstm import fused_lstm_scan, pack_mfma_b

    d, _, _ = refs(hidden, T, B)
    saving = fused_lstm_scan(*device_inputs(d, True))
    assert saving[0].grad_fn is not None
    X, nd, h0, c0, w = device_inputs(d, False)
    with torch.no_grad():
        plain = fused_lstm_scan(X, nd, h0, c0, w.requires_grad_())
    assert all(t.grad_fn is None for t in plain)
    for name, a, b in zip(("H", "hT", "cT"), plain, saving):
        assert torch.equal(a, b.detach()), name
    packed = pack_mfma_b(w.detach().to(BF16).t().contiguous())
    assert len(_kernels.lstm_wide_fwd(X, nd, h0, c0, packed, False)) == 3
    assert len(_kernels.lstm_wide_fwd(X, nd, h0, c0, packed, True)) == 5


@gpu
@requires_gpu
def test_model_route_512(monkeypatch):
    """AtariNet with a 512-unit core: fused scan vs the per-step nn.LSTM loop.
    (A route check; the values of this route, state and gradients included,
    are held to float64 in tests/test_core_composed.py.)"""
    from moolib_amd.models.atari import AtariNet

    torch.manual_seed(7)
    model = AtariNet(num_actions=6, use_lstm=True, lstm_size=512).to("cuda").to(BF16)
    T, B = 3, 2
    done = torch.zeros(T, B, dtype=torch.bool, device="cuda")
    done[1, 0] = True
    inputs = {
        "state": torch.randint(0, 256, (T, B, 4, 84, 84), dtype=torch.uint8, device="cuda"),
        "reward": torch.randn(T, B, device="cuda"),
        "done": done,
        "prev_action": torch.randint(0, 6, (T, B), device="cuda"),
    }
    core = tuple(t.cuda().to(BF16) for t in model.initial_state(batch_size=B))
    with torch.no_grad():
        out_fused, cs_fused = model(inputs, core)
        monkeypatch.setenv("MOOLIB_AMD_NO_LSTM_KERNEL", "1")
        out_loop, _ = model(inputs, core)
    diff = (out_fused["policy_logits"] - out_loop["policy_logits"]).abs().max().item()
    assert diff <= 0.15, diff
    assert [tuple(s.shape) for s in cs_fused] == [(1, B, 512)] * 2


def test_lstm_size_interface():
    from moolib_amd.models.atari import AtariNet, create_model

    wide = AtariNet(num_actions=6, use_lstm=True, lstm_size=512)
    assert wide.core.hidden_size == 512
    assert wide.policy.in_features == wide.baseline.in_features == 512
    state = wide.initial_state(3)
    assert len(state) == 2
    assert all(s.shape == (1, 3, 512) and not s.any() for s in state)
    assert create_model(num_actions=6, use_lstm=True, lstm_size=128).core.hidden_size == 128

    # the default module is today's: same keys, same shapes, in the same order
    default = {k: tuple(v.shape) for k, v in AtariNet(num_actions=6, use_lstm=True).state_dict().items()}
    core = {"core.weight_ih_l0": (1024, 263), "core.weight_hh_l0": (1024, 256),
            "core.bias_ih_l0": (1024,), "core.bias_hh_l0": (1024,),
            "policy.weight": (6, 256), "policy.bias": (6,),
            "baseline.weight": (1, 256), "baseline.bias": (1,)}
    assert list(default)[-8:] == list(core)
    assert {k: default[k] for k in core} == core
    assert default["fc.weight"] == (256, 3872) and len(default) == 40


@gpu
@requires_gpu
@pytest.mark.parametrize("why", ["hidden size 64", "X not contiguous", "h0 dtype",
                                 "packed weight size"])
def test_wide_fwd_rejects(why):
    from moolib_amd import _kernels

    T, B, Hd = 2, 3, 128
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda")
    X, nd, h0, c0 = z(T, B, 4 * Hd, dt=BF16), z(T, B), z(B, Hd, dt=BF16), z(B, Hd)
    wp = z(4 * Hd * Hd, dt=BF16)
    bad = {
        "hidden size 64": (z(T, B, 256, dt=BF16), nd, z(B, 64, dt=BF16), z(B, 64),
                           z(4 * 64 * 64, dt=BF16)),
        "X not contiguous": (z(B, T, 4 * Hd, dt=BF16).transpose(0, 1), nd, h0, c0, wp),
        "h0 dtype": (X, nd, z(B, Hd), c0, wp),
        "packed weight size": (X, nd, h0, c0, wp[:-8]),
    }
    _kernels.lstm_wide_fwd(X, nd, h0, c0, wp, False)  # the accepted form
    with pytest.raises(RuntimeError):
        _kernels.lstm_wide_fwd(*bad[why], False)
