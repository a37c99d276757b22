"""Edge-shape tests of the HIP kernels against fp64 CPU references.

Two kinds (docs/KERNEL_TESTS.md has the arguments and the recorded figures):

* integer-exact: the linear / piecewise-linear kernels get small-integer
  inputs, so fp32 accumulation is exact in any order and the result must be
  `torch.equal` to the fp64 reference cast to the output dtype;
* float: against an fp64 reference with a bound derived from the number
  formats (conv, conv1, LSTM) or recorded from the kernel's own error
  against fp64 and capped by the older fp32-reference tolerance (loss,
  V-trace).

The first part (TestReferences) needs no GPU: it checks the references in
tests/kernel_refs.py against torch's fp64 CPU ops, the integer generators,
the LSTM rounding emulation and the channel-sum launch arithmetic.
"""
import itertools
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import kernel_refs as R

gpu = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

BF16 = torch.bfloat16


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _nhwc(t, dtype=BF16):
    """CPU NCHW fp64 -> GPU channels_last tensor of `dtype`."""
    return t.to(dtype).cuda().contiguous(memory_format=torch.channels_last)


def _figure(**kw):
    """One machine-readable line per measured figure (shown with pytest -s)."""
    print("KERNEL_EDGES_FIGURE " + json.dumps(kw))


# ------------------------------------------------------------------- cases

CONV_SHAPES = [(1, 16, 1, 1), (1, 8, 2, 3), (2, 16, 5, 7), (3, 32, 4, 17)]
CONV_LDS_SHAPES = [(2, 16, 5, 37), (1, 32, 4, 6), (1, 16, 3, 5)]
DGRAD_SHAPES = [(2, 5, 7), (1, 3, 11)]
DGRAD_CK = [(16, 32), (32, 16), (32, 32)]
WGRAD_SHAPES = [(2, 5, 7), (1, 3, 33), (3, 9, 6)]
WGRAD_C = [4, 8, 16, 32]

# prologue x epilogue: every combination the kernel implements
CONV_PROLOGUES = [(), ("relu_in",), ("relu_in", "bias_in")]
CONV_EPILOGUES = [(0,), (1, "bias1"), (2, "bias1"), (3, "bias1", "res"),
                  (3, "bias1", "res", "bias2")]
CONV_COMBOS = list(itertools.product(CONV_PROLOGUES, CONV_EPILOGUES))


def conv_case(seed, N, C, H, W, K, integer=True):
    """Operands of one fused-conv case as bf16-representable fp64 CPU tensors."""
    g = _gen(seed)
    if integer:
        return {
            "x": R.int_tensor(g, (N, C, H, W), -2, 2),
            "w": R.int_tensor(g, (K, C, 3, 3), -1, 1),
            "bias_in": R.int_tensor(g, (C,), -3, 3),
            "bias1": R.int_tensor(g, (K,), -3, 3),
            "bias2": R.int_tensor(g, (K,), -3, 3),
            "res": R.int_tensor(g, (N, K, H, W), -3, 3),
        }
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return {
        "x": R.bf16_round(rn(N, C, H, W)),
        "w": R.bf16_round(rn(K, C, 3, 3) * 0.2),
        "bias_in": R.bf16_round(rn(C) * 0.5),
        "bias1": R.bf16_round(rn(K) * 0.5),
        "bias2": R.bf16_round(rn(K) * 0.5),
        "res": R.bf16_round(rn(N, K, H, W)),
    }


def conv_combo_kwargs(case, combo, tensors=lambda t: t):
    """kwargs for conv3x3 / conv3x3_fused_ref from a (prologue, epilogue) combo."""
    pro, epi = combo
    kw = {"epi": epi[0]}
    if "relu_in" in pro:
        kw["relu_in"] = True
    for name in list(pro) + list(epi[1:]):
        if name != "relu_in":
            kw[name] = tensors(case[name])
    return kw


def dgrad_case(N, H, W, C, K):
    g = _gen(N + C + H + W + K)
    return R.int_tensor(g, (N, K, H, W), -2, 2), R.int_tensor(g, (K, C, 3, 3), -1, 1)


def wgrad_case(N, C, H, W, K):
    g = _gen(N + C + H + W + K)
    return R.int_tensor(g, (N, C, H, W), -2, 2), R.int_tensor(g, (N, K, H, W), -2, 2)


BIAS_SMALL = [(2, C, 3, 5) for C in (8, 16, 24, 32, 40, 48, 56, 64)]
# just past the grid-stride threshold N*H*W*C/8 > 65536 (the loop iterates)
BIAS_LARGE = [(16, 8, 64, 65), (16, 16, 40, 41), (16, 24, 40, 40), (9, 32, 40, 41),
              (10, 40, 37, 41), (12, 48, 32, 32), (9, 56, 33, 35), (3, 64, 52, 53)]


def bias_case(seed, shape):
    g = _gen(seed)
    C = shape[1]
    return {
        "x": R.int_tensor(g, shape, -2, 2),
        "s": R.int_tensor(g, shape, -2, 2),
        "dy": R.int_tensor(g, shape, -3, 3),
        "b1": R.int_tensor(g, (C,), -3, 3),
        "b2": R.int_tensor(g, (C,), -3, 3),
    }


POOL_SHAPES = [(2, 8, 5, 7), (1, 8, 1, 1), (1, 16, 2, 3), (2, 8, 6, 4), (1, 8, 1, 9)]


def pool_case(seed, shape):
    g = _gen(seed)
    N, C, H, W = shape
    x = torch.randint(-2, 3, shape, generator=g).double()
    gout = R.int_tensor(g, (N, C, (H + 1) // 2, (W + 1) // 2), -3, 3)
    return x, gout


def pool_torch_ref(x, gout):
    """CPU F.max_pool2d in fp64 and its autograd gradient."""
    xr = x.double().clone().requires_grad_()
    y = F.max_pool2d(xr, 3, stride=2, padding=1)
    y.backward(gout.double())
    return y.detach(), xr.grad


def _same_with_nan(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(
        torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


LSTM_CASES = [(1, 1), (3, 33), (5, 70)]
# tolerances of the older fp32-reference tests (tests/test_gpu.py TestFusedLSTM):
# (absolute, fraction of max|reference|)
LSTM_PRESENT = {"H": (3e-2, 0.0), "hT": (3e-2, 0.0), "cT": (3e-2, 0.0), "dX": (5e-2, 0.05),
                "dh0": (1e-1, 0.05), "dc0": (1e-1, 0.05), "dW": (2.0, 0.05)}

_lstm_cache = {}


def lstm_refs(T, B):
    """(inputs, R_exact, R_emul), computed once per case and shared."""
    if (T, B) not in _lstm_cache:
        d = R.lstm_inputs(_gen(1000 + T * 100 + B), T, B)
        _lstm_cache[(T, B)] = (d, R.lstm_exact(d), R.lstm_emul(d))
    return _lstm_cache[(T, B)]


LOSS_SHAPES = [(1, 1, 1), (1, 7, 2), (3, 5, 6), (2, 3, 64), (2, 3, 65), (1, 5, 130)]
LOSS_SCALES = [2.0, 25.0]
LOSS_COSTS = [(0.0006, 0.5), (0.01, 1.0)]
LOSS_NAMES = ("pg", "baseline", "entropy", "grad_logits", "grad_baseline")
# today's tolerance (tests/test_gpu.py TestFusedLoss, torch.allclose defaults):
# |got - ref| <= atol + 1e-5 |ref|, atol 1e-4 for losses, 1e-5 for gradients
LOSS_ATOL = {"pg": 1e-4, "baseline": 1e-4, "entropy": 1e-4, "grad_logits": 1e-5,
             "grad_baseline": 1e-5}


def loss_case(T, B, A, scale, seed=0):
    g = _gen(7000 + seed + T * 1000 + B * 100 + A)
    return {
        "logits": (torch.randn(T, B, A, generator=g) * scale),
        "baseline": torch.randn(T, B, generator=g),
        "actions": torch.randint(0, A, (T, B), generator=g),
        "pg_adv": torch.randn(T, B, generator=g),
        "vs": torch.randn(T, B, generator=g),
    }


VTRACE_SHAPES = [(1, 1), (5, 3), (7, 257)]
VTRACE_CLIPS = [(None, None), (0.7, 2.5), (1.0, None)]


def vtrace_case(T, B):
    g = _gen(9000 + T * 1000 + B)
    return {
        "log_rhos": torch.randn(T, B, generator=g) * 1.5,
        "discounts": (torch.rand(T, B, generator=g) > 0.05).float() * 0.99,
        "rewards": torch.randn(T, B, generator=g),
        "values": torch.randn(T, B, generator=g),
        "bootstrap": torch.randn(B, generator=g),
    }


# Recorded on an MI355X (docs/KERNEL_TESTS.md): max |kernel - fp64| per case.
# The test bound is 4x this (fast exp/log and the atomic summation order vary
# from run to run), floored at 4 * 2**-24 * max|ref| - for the summed
# policy-gradient loss, whose terms cancel, 4 * 2**-24 * mean|terms| - since
# an error below one fp32 rounding of the operands is luck, not accuracy, and
# capped elementwise by today's atol + 1e-5|ref|.
LOSS_MEASURED = {
    (1, 1, 1, 2.0, 0.0006): {"pg": 0, "baseline": 1.5e-09, "entropy": 0, "grad_logits": 0, "grad_baseline": 0},
    (1, 1, 1, 2.0, 0.01): {"pg": 0, "baseline": 3.01e-09, "entropy": 0, "grad_logits": 0, "grad_baseline": 0},
    (1, 1, 1, 25.0, 0.0006): {"pg": 0, "baseline": 1.5e-09, "entropy": 0, "grad_logits": 0, "grad_baseline": 0},
    (1, 1, 1, 25.0, 0.01): {"pg": 0, "baseline": 3.01e-09, "entropy": 0, "grad_logits": 0, "grad_baseline": 0},
    (1, 7, 2, 2.0, 0.0006): {"pg": 1.28e-07, "baseline": 3.02e-08, "entropy": 1.99e-11, "grad_logits": 1.35e-08, "grad_baseline": 8.51e-09},
    (1, 7, 2, 2.0, 0.01): {"pg": 8.52e-09, "baseline": 6.04e-08, "entropy": 7.57e-11, "grad_logits": 1.35e-08, "grad_baseline": 1.7e-08},
    (1, 7, 2, 25.0, 0.0006): {"pg": 2.28e-06, "baseline": 3.02e-08, "entropy": 7.48e-12, "grad_logits": 1.95e-08, "grad_baseline": 8.51e-09},
    (1, 7, 2, 25.0, 0.01): {"pg": 2.28e-06, "baseline": 6.04e-08, "entropy": 1.25e-10, "grad_logits": 1.95e-08, "grad_baseline": 1.7e-08},
    (3, 5, 6, 2.0, 0.0006): {"pg": 6.16e-08, "baseline": 5.15e-08, "entropy": 1.05e-10, "grad_logits": 1.22e-08, "grad_baseline": 1.24e-08},
    (3, 5, 6, 2.0, 0.01): {"pg": 2.03e-09, "baseline": 1.62e-08, "entropy": 1.97e-10, "grad_logits": 1.29e-08, "grad_baseline": 2.48e-08},
    (3, 5, 6, 25.0, 0.0006): {"pg": 4.44e-07, "baseline": 5.15e-08, "entropy": 7.34e-11, "grad_logits": 3.7e-08, "grad_baseline": 1.24e-08},
    (3, 5, 6, 25.0, 0.01): {"pg": 4.44e-07, "baseline": 1.03e-07, "entropy": 1.24e-09, "grad_logits": 3.7e-08, "grad_baseline": 2.48e-08},
    (2, 3, 64, 2.0, 0.0006): {"pg": 4.09e-08, "baseline": 4.05e-08, "entropy": 3.25e-10, "grad_logits": 8.87e-09, "grad_baseline": 7.45e-09},
    (2, 3, 64, 2.0, 0.01): {"pg": 4.09e-08, "baseline": 2e-07, "entropy": 9.3e-11, "grad_logits": 7.05e-09, "grad_baseline": 1.49e-08},
    (2, 3, 64, 25.0, 0.0006): {"pg": 2.67e-07, "baseline": 1e-07, "entropy": 2.24e-10, "grad_logits": 1.21e-07, "grad_baseline": 7.45e-09},
    (2, 3, 64, 25.0, 0.01): {"pg": 2.67e-07, "baseline": 8.09e-08, "entropy": 4e-09, "grad_logits": 1.08e-07, "grad_baseline": 1.49e-08},
    (2, 3, 65, 2.0, 0.0006): {"pg": 8.24e-08, "baseline": 1.37e-07, "entropy": 1.27e-10, "grad_logits": 1.82e-08, "grad_baseline": 1.99e-08},
    (2, 3, 65, 2.0, 0.01): {"pg": 8.24e-08, "baseline": 3.6e-08, "entropy": 8.71e-10, "grad_logits": 1.97e-08, "grad_baseline": 3.97e-08},
    (2, 3, 65, 25.0, 0.0006): {"pg": 8.21e-07, "baseline": 1.8e-08, "entropy": 3.47e-10, "grad_logits": 1.63e-07, "grad_baseline": 1.99e-08},
    (2, 3, 65, 25.0, 0.01): {"pg": 8.21e-07, "baseline": 3.6e-08, "entropy": 5.8e-09, "grad_logits": 1.65e-07, "grad_baseline": 3.97e-08},
    (1, 5, 130, 2.0, 0.0006): {"pg": 8.44e-08, "baseline": 3.79e-08, "entropy": 2.32e-10, "grad_logits": 3.17e-08, "grad_baseline": 5.96e-09},
    (1, 5, 130, 2.0, 0.01): {"pg": 8.44e-08, "baseline": 7.58e-08, "entropy": 1.1e-11, "grad_logits": 2.73e-08, "grad_baseline": 1.19e-08},
    (1, 5, 130, 25.0, 0.0006): {"pg": 9.82e-07, "baseline": 3.79e-08, "entropy": 4.78e-11, "grad_logits": 1.33e-07, "grad_baseline": 5.96e-09},
    (1, 5, 130, 25.0, 0.01): {"pg": 2.89e-06, "baseline": 7.58e-08, "entropy": 8.93e-10, "grad_logits": 1.34e-07, "grad_baseline": 1.19e-08},
    ('grad_scale', 3.0): {"grad_logits": 3.86e-08, "grad_baseline": 2.98e-08},
    ('total', 'contiguous_int32_actions'): {"total": 1.13e-07, "grad_logits": 4.05e-08, "grad_baseline": 1.79e-08},
    ('total', 'transposed_logits'): {"total": 1.13e-07, "grad_logits": 4.05e-08, "grad_baseline": 1.79e-08},
}
VTRACE_MEASURED = {
    (1, 1, 'None', 'None'): {"vs": 2.13e-08, "pg_advantages": 3.83e-08},
    (1, 1, '0.7', '2.5'): {"vs": 2.13e-08, "pg_advantages": 3.83e-08},
    (1, 1, '1.0', 'None'): {"vs": 2.13e-08, "pg_advantages": 3.83e-08},
    (5, 3, 'None', 'None'): {"vs": 7.9e-07, "pg_advantages": 1.07e-05},
    (5, 3, '0.7', '2.5'): {"vs": 2.19e-07, "pg_advantages": 3.59e-07},
    (5, 3, '1.0', 'None'): {"vs": 1.6e-07, "pg_advantages": 1.78e-06},
    (7, 257, 'None', 'None'): {"vs": 4.37e-05, "pg_advantages": 0.000738},
    (7, 257, '0.7', '2.5'): {"vs": 5.42e-07, "pg_advantages": 1.55e-06},
    (7, 257, '1.0', 'None'): {"vs": 8.68e-07, "pg_advantages": 2.05e-05},
}


def _recorded_bound(table, key, name, got, ref, atol, e_ref, sum_scale=None):
    """Check |got - ref| against 4x the recorded kernel error (see above).
    `sum_scale` is sum|terms| where the value is an fp32 sum whose terms
    cancel (the floor then follows the terms, not the smaller result).
    Returns the list of violations, so a test reports every tensor at once."""
    err = (got.double() - ref).abs()
    scale = ref.abs().max().item() if sum_scale is None else sum_scale
    measured = table.get(key, {}).get(name)
    worst = err.max().item()
    bound = None if measured is None else 4 * max(measured, R.F32_EPS * scale)
    _figure(kind="recorded", case=list(key), tensor=name, e_ref=e_ref, err=worst, bound=bound,
            scale=scale)
    bad = []
    if not (err <= atol + 1e-5 * ref.abs()).all():
        bad.append((key, name, worst, "over today's tolerance", atol))
    if measured is None:
        bad.append((key, name, "no recorded kernel error for this case"))
    elif worst > bound:
        bad.append((key, name, worst, "over 4x the recorded error", bound))
    return bad


# ===================================================== CPU self-checks (no GPU)


class TestReferences:
    """The fp64 references agree with torch's own CPU fp64 ops; runs anywhere."""

    @pytest.mark.parametrize("shape,K", [((2, 8, 5, 7), 16), ((1, 4, 3, 33), 32),
                                         ((3, 32, 1, 1), 16), ((1, 16, 2, 3), 32)])
    def test_conv_refs_match_torch(self, shape, K):
        g = _gen(11)
        x = torch.randn(*shape, generator=g, dtype=torch.float64)
        w = torch.randn(K, shape[1], 3, 3, generator=g, dtype=torch.float64)
        dy = torch.randn(shape[0], K, *shape[2:], generator=g, dtype=torch.float64)
        assert torch.allclose(R.conv3x3_ref(x, w), F.conv2d(x, w, None, padding=1),
                              rtol=1e-12, atol=1e-12)
        dx, dw, _ = torch.ops.aten.convolution_backward(
            dy, x, w, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1, [True, True, False])
        assert torch.allclose(R.conv3x3_dgrad_ref(dy, w), dx, rtol=1e-12, atol=1e-12)
        assert torch.allclose(R.conv3x3_wgrad_ref(x, dy), dw, rtol=1e-12, atol=1e-12)

    def test_fused_conv_ref_matches_torch(self):
        case = conv_case(5, 2, 16, 5, 7, 32, integer=False)
        for combo in CONV_COMBOS:
            kw = conv_combo_kwargs(case, combo)
            x = case["x"]
            if kw.get("relu_in"):
                if "bias_in" in kw:
                    x = x + case["bias_in"].view(1, -1, 1, 1)
                x = R.bf16_round(torch.relu(x))
            y = F.conv2d(x, case["w"], None, padding=1)
            v = lambda n: case[n].view(1, -1, 1, 1)
            if kw["epi"] >= 1:
                y = y + v("bias1")
            if kw["epi"] == 2:
                y = torch.relu(y)
            if kw["epi"] == 3:
                y = y + case["res"] + (v("bias2") if "bias2" in kw else 0)
            assert torch.allclose(R.conv3x3_fused_ref(case["x"], case["w"], **kw), y,
                                  rtol=1e-12, atol=1e-12), combo

    @pytest.mark.parametrize("shape", POOL_SHAPES + [(2, 8, 5, 7)])
    def test_pool_ref_matches_torch(self, shape):
        """First maximum in row-major scan order, on tie-heavy inputs."""
        x, gout = pool_case(sum(shape), shape)
        y, gin = R.maxpool3x3s2_ref(x, gout)
        y_t, gin_t = pool_torch_ref(x, gout)
        assert torch.equal(y, y_t)
        assert torch.equal(gin, gin_t)

    def test_pool_ref_nan_and_inf_match_torch(self):
        x, gout = pool_case(3, (2, 8, 5, 7))
        x[1, 3, 3, 5] = float("nan")
        y, gin = R.maxpool3x3s2_ref(x, gout)
        y_t, gin_t = pool_torch_ref(x, gout)
        assert torch.isnan(y).sum() == 4  # row 3 and column 5 each lie in two windows
        assert _same_with_nan(y, y_t) and torch.equal(gin, gin_t)
        x = torch.full((1, 8, 3, 3), float("-inf"), dtype=torch.float64)
        gout = R.int_tensor(_gen(4), (1, 8, 2, 2), 1, 3)
        y, gin = R.maxpool3x3s2_ref(x, gout)
        y_t, gin_t = pool_torch_ref(x, gout)
        assert torch.equal(y, y_t) and torch.equal(gin, gin_t)
        assert gin.sum() == gout.sum()  # no window lost its gradient

    @pytest.mark.parametrize("shape", POOL_SHAPES)
    def test_pool_inputs_tie(self, shape):
        """randint(-2, 3) makes ties the rule, not an accident. A window of n
        elements from 5 values ties with probability 0 (n=1), .20, .52, .36,
        .50, .67 (n=2,3,4,6,9), so 'most windows tie' is out of reach at
        these shapes (48% expected at (2,8,5,7), none at 1x1). Every window
        that CAN tie does so with probability >= .20: require that fraction."""
        x, _ = pool_case(sum(shape), shape)
        frac = R.maxpool_tie_fraction(x)
        if shape[2] * shape[3] > 1:
            assert frac >= 0.2, frac

    def test_integer_generators_stay_exact(self):
        """Every reference value (and every partial sum: bounded by sum|terms|)
        of the integer cases is an integer far below 2**24."""
        for (N, C, H, W), K in itertools.product(CONV_SHAPES + CONV_LDS_SHAPES, (16, 32)):
            case = conv_case(N + C + H + W + K, N, C, H, W, K)
            for combo in CONV_COMBOS:
                y, S = R.conv3x3_fused_ref(case["x"], case["w"], return_scale=True,
                                           **conv_combo_kwargs(case, combo))
                R.assert_int_exact(y, S)
                assert y.abs().max() <= 256  # bf16 holds these integers exactly
        for (N, H, W), (C, K) in itertools.product(DGRAD_SHAPES, DGRAD_CK):
            dy, w = dgrad_case(N, H, W, C, K)
            R.assert_int_exact(R.conv3x3_dgrad_ref(dy, w), R.conv3x3_dgrad_ref(dy.abs(), w.abs()))
            assert R.conv3x3_dgrad_ref(dy, w).abs().max() <= 256
        for (N, H, W), C, K in itertools.product(WGRAD_SHAPES + [(4, 20, 9)], WGRAD_C, (16, 32)):
            x, dy = wgrad_case(N, C, H, W, K)
            R.assert_int_exact(R.conv3x3_wgrad_ref(x, dy), R.conv3x3_wgrad_ref(x.abs(), dy.abs()))
        for shape in BIAS_SMALL + BIAS_LARGE:
            c = bias_case(sum(shape), shape)
            R.assert_int_exact(c["dy"].abs().sum(dim=(0, 2, 3)))
            assert (c["x"].abs() + c["s"].abs() + c["b1"].abs().max() + c["b2"].abs().max()).max() <= 256

    def test_lstm_emulation_off_equals_exact(self):
        for T, B in [(1, 1), (3, 5), (4, 33)]:
            d = R.lstm_inputs(_gen(T * 10 + B), T, B)
            exact, plain = R.lstm_exact(d), R.lstm_emul(d, rounding=False)
            for k in R.LSTM_TENSORS:
                assert torch.allclose(plain[k], exact[k], rtol=1e-10, atol=1e-12), (T, B, k)

    @pytest.mark.parametrize("T,B", LSTM_CASES)
    def test_lstm_rounding_distance(self, T, B):
        """d = max|R_emul - R_exact| is non-zero (the rounding points matter)
        and the bound built from it is tighter than the older tolerance."""
        d, exact, emul = lstm_refs(T, B)
        assert d["nd"][0, 0] == 0 and (B < 2 or d["nd"][:, 1].sum() == 0)
        assert B < 3 or d["nd"][:, 2].sum() == T
        for k, (dist, bound) in R.lstm_bounds(exact, emul).items():
            atol, rel = LSTM_PRESENT[k]
            present = atol + rel * exact[k].abs().max().item()
            _figure(kind="lstm_d", case=[T, B], tensor=k, d=dist, bound=bound, present=present,
                    scale=exact[k].abs().max().item())
            # (1,1): the only row is done at t=0, so nothing recurrent is
            # rounded and several tensors are exactly zero in both references
            assert dist > 0 or (T, B) == (1, 1), k
            assert bound < present, (k, bound, present)

    def test_channel_sum_mapping(self):
        """Pure-Python model of the channel-sum thread -> channel mapping:
        with the rounded grid every octet is credited to its own channel,
        for every accepted C at the tested shapes; without the rounding the
        C = 24, 40, 48, 56 shapes past the grid-stride threshold are not."""
        for N, C, H, W in BIAS_SMALL + BIAS_LARGE:
            total8, c8n = N * C * H * W // 8, C // 8
            blocks = R.channel_sum_blocks(total8, c8n)
            assert blocks >= 1
            assert R.channel_sum_miscredited(total8, c8n, blocks) == 0, (N, C, H, W)
            old = R.channel_sum_blocks_unrounded(total8, c8n)
            if C in (8, 16, 32, 64):
                assert blocks == old  # launch geometry unchanged
            bad_before = R.channel_sum_miscredited(total8, c8n, old)
            assert (bad_before > 0) == (C in (24, 40, 48, 56) and total8 > 65536), (N, C, H, W)
        # any size, any accepted C, and the block-cap override too
        for c8n in range(1, 9):
            for total8 in (1, 255, 65536, 65537, 200000, 3000 * 768 + 5):
                for cap in (None, 1, 2, 7, 300):
                    blocks = R.channel_sum_blocks(total8, c8n, cap=cap)
                    assert R.channel_sum_miscredited(total8, c8n, blocks) == 0

    def test_loss_and_vtrace_refs_match_project_cpu_paths(self):
        from moolib_amd.ops import vtrace

        c = loss_case(3, 5, 6, 2.0)
        ref = R.impala_loss_ref(c["logits"], c["actions"], c["pg_adv"], c["vs"], c["baseline"],
                                0.01, 0.5)
        eager = R.impala_loss_eager(c["logits"], c["actions"], c["pg_adv"], c["vs"],
                                    c["baseline"], 0.01, 0.5)
        for a, b in zip(ref, eager):
            assert torch.allclose(a, b.double(), atol=1e-6)
        v = vtrace_case(5, 3)
        for clips in VTRACE_CLIPS:
            vs, pg = R.vtrace_ref(*v.values(), *clips)
            cpu = vtrace.from_importance_weights(
                *(t.double() for t in v.values()), clip_rho_threshold=clips[0],
                clip_pg_rho_threshold=clips[1])
            assert torch.allclose(vs, cpu.vs, rtol=1e-12, atol=1e-12)
            assert torch.allclose(pg, cpu.pg_advantages, rtol=1e-12, atol=1e-12)


# ============================================================ integer-exact


def _conv_gpu(case, K, combo, rt=0):
    from moolib_amd.ops import conv3x3 as c3

    to_gpu = lambda t: _nhwc(t) if t.dim() == 4 else t.to(BF16).cuda()
    kw = conv_combo_kwargs(case, combo, to_gpu)
    wp = c3.pack_weight(case["w"].to(BF16)).cuda()
    return c3.conv3x3(_nhwc(case["x"]), wp, K, rt=rt, **kw).cpu()


@gpu
@requires_gpu
class TestConv3x3Exact:
    @pytest.mark.parametrize("K", [16, 32])
    @pytest.mark.parametrize("shape", CONV_SHAPES)
    def test_flat_kernel_every_fusion(self, shape, K):
        N, C, H, W = shape
        case = conv_case(N + C + H + W + K, N, C, H, W, K)
        for combo in CONV_COMBOS:
            ref = R.conv3x3_fused_ref(case["x"], case["w"], **conv_combo_kwargs(case, combo))
            assert ref.abs().max() <= 256
            for rt in (1, 2, 4):
                got = _conv_gpu(case, K, combo, rt)
                assert got.dtype == BF16 and got.shape == ref.shape
                assert torch.equal(got, ref.to(BF16)), (shape, K, combo, rt)

    def test_float_case(self):
        """Random floats: rounding behaviour. Bound per element: one bf16 step
        of the output plus the fp32 accumulation bound over the 9C taps and
        the epilogue terms, with a factor 2 of slack."""
        N, C, H, W, K = 3, 32, 4, 17, 32
        case = conv_case(77, N, C, H, W, K, integer=False)
        for combo in CONV_COMBOS:
            ref, S = R.conv3x3_fused_ref(case["x"], case["w"], return_scale=True,
                                         **conv_combo_kwargs(case, combo))
            got = _conv_gpu(case, K, combo).double()
            bound = R.BF16_STEP * ref.abs() + 2 * R.fp32_accum_bound(9 * C + 4, S)
            err = (got - ref).abs()
            _figure(kind="derived", test="conv3x3_float", case=[str(combo)],
                    err_over_bound=(err / bound).max().item())
            assert (err <= bound).all(), (combo, (err / bound).max().item())

    @pytest.mark.parametrize("C,K", DGRAD_CK)
    @pytest.mark.parametrize("shape", DGRAD_SHAPES)
    def test_dgrad_pack(self, shape, C, K):
        from moolib_amd.ops import conv3x3 as c3

        N, H, W = shape
        dy, w = dgrad_case(N, H, W, C, K)
        ref = R.conv3x3_dgrad_ref(dy, w)
        assert ref.abs().max() <= 256
        got = c3.conv3x3(_nhwc(dy), c3.pack_weight_dgrad(w.to(BF16)).cuda(), C).cpu()
        assert torch.equal(got, ref.to(BF16)), (shape, C, K)


_LDS_SCRIPT = """
import itertools, sys, torch
import kernel_refs as R
import test_kernel_edges as E
from moolib_amd.ops import conv3x3 as c3
for (N, C, H, W), K in itertools.product(E.CONV_LDS_SHAPES, (16, 32)):
    case = E.conv_case(N + C + H + W + K, N, C, H, W, K)
    for combo in E.CONV_COMBOS:
        ref = R.conv3x3_fused_ref(case["x"], case["w"], **E.conv_combo_kwargs(case, combo))
        assert ref.abs().max() <= 256
        got = E._conv_gpu(case, K, combo)  # rt=0: the LDS variant where it applies
        assert torch.equal(got, ref.to(torch.bfloat16)), ((N, C, H, W), K, combo)
print("OK")
"""


@gpu
@requires_gpu
class TestConv3x3LdsExact:
    def test_lds_variant_matches_fp64(self):
        """LDS band-slab kernel against the fp64 reference itself (subprocess:
        the variant gate is read once per process). (1,16,3,5) has H=3, where
        the host falls back to the flat kernel; only correctness is asserted."""
        repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        env = dict(os.environ, MOOLIB_AMD_CONV3_LDS="1")
        env["PYTHONPATH"] = os.pathsep.join(
            [repo, os.path.join(repo, "tests"), env.get("PYTHONPATH", "")])
        r = subprocess.run([sys.executable, "-c", _LDS_SCRIPT], capture_output=True, text=True,
                           timeout=170, env=env, cwd=repo)
        assert r.returncode == 0 and "OK" in r.stdout, r.stderr[-2000:]


@gpu
@requires_gpu
class TestWgradExact:
    def _check(self, N, C, H, W, K):
        from moolib_amd import _kernels

        x, dy = wgrad_case(N, C, H, W, K)
        out = _kernels.wgrad3x3_nhwc(_nhwc(x), _nhwc(dy)).cpu()
        assert out.dtype == torch.float32 and out.shape == ((9 * C + 15) // 16 * 16, K)
        got = out[: 9 * C].view(3, 3, C, K).permute(3, 2, 0, 1).double()
        assert torch.equal(got, R.conv3x3_wgrad_ref(x, dy)), (N, C, H, W, K)
        assert out[9 * C:].abs().sum() == 0  # GEMM rows past 9C stay zero

    @pytest.mark.parametrize("K", [16, 32])
    @pytest.mark.parametrize("C", WGRAD_C)
    def test_shapes(self, C, K):
        for N, H, W in WGRAD_SHAPES:
            self._check(N, C, H, W, K)

    def test_uneven_slabs_per_block(self, monkeypatch):
        """3 blocks share the slabs unevenly and each restages several times."""
        monkeypatch.setenv("MOOLIB_AMD_WGRAD_BLOCKS", "3")
        self._check(4, 16, 20, 9, 16)
        self._check(4, 16, 20, 9, 32)


@gpu
@requires_gpu
class TestBiasKernelsExact:
    @pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
    @pytest.mark.parametrize("shape", BIAS_SMALL + BIAS_LARGE)
    def test_forward_dx_db(self, shape, dtype):
        from moolib_amd import _kernels
        from moolib_amd.ops import fused_bias

        c = bias_case(sum(shape), shape)
        C = shape[1]
        x, s, dy = (_nhwc(c[k], dtype) for k in ("x", "s", "dy"))
        b1, b2 = (c[k].to(dtype).cuda() for k in ("b1", "b2"))
        assert fused_bias.available(x)
        v = lambda b: b.view(1, -1, 1, 1)

        y_ref = torch.relu(c["x"] + v(c["b1"]))
        y = _kernels.bias_relu_fwd(x, b1)
        assert y.dtype == dtype and torch.equal(y.cpu(), y_ref.to(dtype))
        dx, db = _kernels.bias_relu_bwd(dy, y)
        dx_ref = c["dy"] * (y_ref > 0)
        assert dx.dtype == dtype and torch.equal(dx.cpu(), dx_ref.to(dtype))
        assert db.dtype == torch.float32 and db.shape == (C,)
        assert torch.equal(db.cpu().double(), dx_ref.sum(dim=(0, 2, 3))), (shape, dtype)

        got = _kernels.channel_sum_fp32(dy)
        assert got.dtype == torch.float32
        assert torch.equal(got.cpu().double(), c["dy"].sum(dim=(0, 2, 3))), (shape, dtype)

        a = _kernels.bias_add2_fwd(x, b1, s, b2).cpu()
        assert torch.equal(a, (c["x"] + v(c["b1"]) + c["s"] + v(c["b2"])).to(dtype))
        a = _kernels.bias_add2_fwd(x, b1, s, None).cpu()
        assert torch.equal(a, (c["x"] + v(c["b1"]) + c["s"]).to(dtype))

    def test_autograd_wrappers(self):
        """bias_relu / bias_add2 through autograd at a C=24 shape past the
        grid-stride threshold: the gradients the optimizer would see."""
        from moolib_amd.ops.fused_bias import bias_add2, bias_relu

        shape = (16, 24, 40, 40)
        c = bias_case(1, shape)
        x, s = (_nhwc(c[k], torch.float32).requires_grad_() for k in ("x", "s"))
        b1, b2 = (c[k].float().cuda().requires_grad_() for k in ("b1", "b2"))
        dy = _nhwc(c["dy"], torch.float32)
        bias_relu(x, b1).backward(dy)
        mask = (c["x"] + c["b1"].view(1, -1, 1, 1)) > 0
        assert torch.equal(b1.grad.cpu().double(), (c["dy"] * mask).sum(dim=(0, 2, 3)))
        b1.grad = None
        bias_add2(x, b1, s, b2).backward(dy)
        for b in (b1, b2):
            assert torch.equal(b.grad.cpu().double(), c["dy"].sum(dim=(0, 2, 3)))


@gpu
@requires_gpu
class TestMaxPoolExact:
    @pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
    @pytest.mark.parametrize("shape", POOL_SHAPES)
    def test_ties_and_gradient_routing(self, shape, dtype):
        from moolib_amd.ops.pool import maxpool3x3s2

        x_cpu, gout = pool_case(sum(shape), shape)
        y_ref, gin_ref = pool_torch_ref(x_cpu, gout)
        x = _nhwc(x_cpu, dtype).requires_grad_()
        y = maxpool3x3s2(x)
        assert y.dtype == dtype and torch.equal(y.detach().cpu(), y_ref.to(dtype))
        y.backward(_nhwc(gout, dtype))
        assert torch.equal(x.grad.cpu(), gin_ref.to(dtype)), (shape, dtype)

    @pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
    def test_nan_propagates(self, dtype):
        from moolib_amd.ops.pool import maxpool3x3s2

        x_cpu, gout = pool_case(3, (2, 8, 5, 7))
        x_cpu[1, 3, 3, 5] = float("nan")
        y_ref, gin_ref = pool_torch_ref(x_cpu, gout)
        x = _nhwc(x_cpu, dtype).requires_grad_()
        y = maxpool3x3s2(x)
        assert torch.isnan(y).sum().item() == 4
        assert _same_with_nan(y.detach().cpu(), y_ref.to(dtype))
        y.backward(_nhwc(gout, dtype))
        assert torch.equal(x.grad.cpu(), gin_ref.to(dtype))

    def test_all_minus_inf_window_keeps_gradient(self):
        from moolib_amd.ops.pool import maxpool3x3s2

        x_cpu = torch.full((1, 8, 3, 3), float("-inf"), dtype=torch.float64)
        gout = R.int_tensor(_gen(4), (1, 8, 2, 2), 1, 3)
        y_ref, gin_ref = pool_torch_ref(x_cpu, gout)
        x = _nhwc(x_cpu, torch.float32).requires_grad_()
        y = maxpool3x3s2(x)
        assert torch.equal(y.detach().cpu().double(), y_ref)
        y.backward(_nhwc(gout, torch.float32))
        assert torch.equal(x.grad.cpu().double(), gin_ref)


def frames_ref(x, scale, pad):
    """The kernel's multiply form, bit for bit; padded channels are zero."""
    N, C, H, W = x.shape
    want = torch.zeros(N, max(pad, C), H, W, dtype=BF16)
    want[:, :C] = (x.float() * torch.tensor(scale, dtype=torch.float32)).bfloat16()
    return want


@gpu
@requires_gpu
class TestFramesExact:
    @pytest.mark.parametrize("shape,pad", [((2, 4, 5, 7), 0), ((2, 4, 5, 7), 8), ((2, 4, 5, 7), 16),
                                           ((1, 1, 3, 2), 8), ((3, 3, 2, 9), 8), ((1, 8, 4, 4), 8)])
    def test_bit_exact(self, shape, pad):
        from moolib_amd import _kernels

        x = torch.randint(0, 256, shape, dtype=torch.uint8, generator=_gen(sum(shape) + pad))
        x[0, 0, 0, :2] = torch.tensor([0, 255], dtype=torch.uint8)
        got = _kernels.frames_u8_to_bf16_nhwc(x.cuda(), 1.0 / 255.0, pad)
        C = shape[1]
        assert got.dtype == BF16 and got.shape == (shape[0], max(pad, C), shape[2], shape[3])
        assert got.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(got.cpu(), frames_ref(x, 1.0 / 255.0, pad))
        assert got[:, C:].abs().sum().item() == 0.0


@gpu
@requires_gpu
class TestBatchedCopyExact:
    def test_53_pairs_mixed(self):
        """Two mid-list flushes (24 descriptors per launch), all three vector
        widths, the grid-stride copy loop, a zero-size pair and an expanded
        source, checked against the same copies done on the CPU - including
        the destination bytes outside each view."""
        from moolib_amd import _kernels

        g = _gen(53)
        pairs = []  # (dst_base, dst_view_fn, src_base, src_view_fn)
        ident = lambda t: t
        for i in range(20):  # contiguous, 16-byte vectors
            pairs.append((torch.zeros(7, 16 + 4 * i), ident,
                          torch.randn(7, 16 + 4 * i, generator=g), ident))
        for i in range(10):  # float32 view from element 1: 4-byte vectors
            n = 9 + i
            pairs.append((torch.zeros(n + 2), lambda t, n=n: t[1 : 1 + n],
                          torch.randn(n + 3, generator=g), lambda t, n=n: t[1 : 1 + n]))
        for i in range(10):  # odd rowBytes: byte path
            pairs.append((torch.zeros(5, 13 + 2 * i, dtype=torch.uint8), ident,
                          torch.randint(0, 255, (5, 13 + 2 * i), dtype=torch.uint8, generator=g),
                          ident))
        for i in range(5):  # bf16, 132 bytes: 4-byte vectors
            pairs.append((torch.zeros(6, 11, dtype=BF16), ident,
                          torch.randn(6, 11, generator=g).to(BF16), ident))
        for i in range(5):  # int64 strided rows (narrow of a wider buffer)
            pairs.append((torch.zeros(4, 10 + i, 3, dtype=torch.int64),
                          lambda t: t.narrow(1, 2, 6),
                          torch.randint(-9, 9, (4, 20, 3), generator=g),
                          lambda t: t.narrow(1, 11, 6)))
        pairs.append((torch.zeros(5, 1024, 1024, dtype=torch.uint8), ident,  # > 1024*256 units
                      torch.randint(0, 255, (5, 1024, 1024), dtype=torch.uint8, generator=g),
                      ident))
        pairs.append((torch.zeros(0, 7), ident, torch.zeros(0, 7), ident))  # zero-size
        pairs.append((torch.zeros(6, 8), ident, torch.randn(1, 8, generator=g),  # stride-0 rows
                      lambda t: t.expand(6, 8)))
        assert len(pairs) == 53
        order = torch.randperm(53, generator=g).tolist()
        pairs = [pairs[i] for i in order]

        want, dst_bases, dsts, srcs = [], [], [], []
        for dbase, dfn, sbase, sfn in pairs:
            w = dbase.clone()
            dfn(w).copy_(sfn(sbase))
            want.append(w)
            db = dbase.cuda()
            dst_bases.append(db)
            dsts.append(dfn(db))
            srcs.append(sfn(sbase.cuda()))
        assert srcs[order.index(52)].stride(0) == 0
        _kernels.batched_copy(dsts, srcs)
        torch.cuda.synchronize()
        for i, (db, w) in enumerate(zip(dst_bases, want)):
            assert torch.equal(db.cpu(), w), order[i]

    def test_repack_23_weights(self):
        """More weights than one launch's descriptor table (20) holds."""
        from moolib_amd import _kernels
        from moolib_amd.ops import conv3x3 as c3

        g = _gen(23)
        specs = [(16, 16), (16, 32), (32, 32), (32, 16), (8, 16), (4, 16)]
        ws, fs, ds, cps, refs = [], [], [], [], []
        for i in range(23):
            C, K = specs[i % len(specs)]
            w = torch.randn(K, C, 3, 3, generator=g).to(BF16)
            pad8 = C == 4 and i % 2 == 1  # the first conv's C=8 zero-padded pack
            f_ref = c3.pack_weight(F.pad(w, (0, 0, 0, 0, 0, 4)) if pad8 else w)
            d_ref = c3.pack_weight_dgrad(w) if C >= 16 else None
            wg = w.cuda()
            if i % 3 == 0:
                wg = wg.to(memory_format=torch.channels_last)
            ws.append(wg)
            fs.append(torch.full_like(f_ref, 7).cuda())
            ds.append(torch.full_like(d_ref, 7).cuda() if d_ref is not None else wg.new_empty(0))
            cps.append(8 if pad8 else 0)
            refs.append((f_ref, d_ref))
        _kernels.repack3x3_batched(ws, fs, ds, cps)
        torch.cuda.synchronize()
        for i, (f_ref, d_ref) in enumerate(refs):
            assert torch.equal(fs[i].cpu(), f_ref), (i, "fwd")
            if d_ref is not None:
                assert torch.equal(ds[i].cpu(), d_ref), (i, "dgrad")


# =================================================== float, fp64 references


@gpu
@requires_gpu
class TestConv1U8:
    @pytest.mark.parametrize("shape", [(2, 4, 6, 7), (1, 4, 1, 1), (1, 4, 3, 4), (2, 4, 2, 5),
                                       (1, 4, 7, 12)])
    def test_against_fp64(self, shape):
        """|got - ref| <= 2**-8 |ref| + 2*40*2**-24 * S, S = sum|x*scale||w| + |b|:
        one bf16 step of the output, plus the fp32 accumulation bound for the
        37 terms and the x*scale rounding with a factor 2 of slack."""
        from moolib_amd import _kernels

        g = _gen(sum(shape))
        x = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
        w = R.bf16_round(torch.randn(16, 4, 3, 3, generator=g, dtype=torch.float64) * 0.3)
        b = R.bf16_round(torch.randn(16, generator=g, dtype=torch.float64) * 0.3)
        ref, S = R.conv1_u8_ref(x, w, b, 1.0 / 255.0)
        wk = w.permute(2, 3, 1, 0).contiguous().to(BF16).cuda()  # [3,3,4,16]
        got = _kernels.conv1_u8_nhwc(x.cuda(), wk, b.to(BF16).cuda(), 1.0 / 255.0)
        assert got.dtype == BF16 and got.shape == ref.shape
        assert got.is_contiguous(memory_format=torch.channels_last)
        err = (got.cpu().double() - ref).abs()
        bound = R.BF16_STEP * ref.abs() + 2 * 40 * R.F32_EPS * S
        _figure(kind="derived", test="conv1_u8", case=list(shape),
                err_over_bound=(err / bound).max().item())
        assert (err <= bound).all(), (shape, (err / bound).max().item())


def _loss_key(T, B, A, scale, ec):
    return (T, B, A, scale, ec)


@gpu
@requires_gpu
class TestImpalaLossFp64:
    @pytest.mark.parametrize("T,B,A", LOSS_SHAPES)
    def test_parts_and_gradients(self, T, B, A):
        from moolib_amd import _kernels

        bad = []
        for scale, (ec, bc) in itertools.product(LOSS_SCALES, LOSS_COSTS):
            c = loss_case(T, B, A, scale)
            args = (c["logits"], c["actions"], c["pg_adv"], c["vs"], c["baseline"], ec, bc)
            ref = R.impala_loss_ref(*args)
            eager = R.impala_loss_eager(*args)
            parts, gl, gb = _kernels.impala_loss(
                *(t.cuda() for t in args[:5]), float(ec), float(bc), 1.0)
            assert gl.shape == (T, B, A) and gb.shape == (T, B)
            got = {"pg": parts[0], "baseline": parts[1], "entropy": parts[2],
                   "grad_logits": gl, "grad_baseline": gb}
            want = {"pg": ref[0][0], "baseline": ref[0][1], "entropy": ref[0][2],
                    "grad_logits": ref[1], "grad_baseline": ref[2]}
            e_ref = {"pg": eager[0][0], "baseline": eager[0][1], "entropy": eager[0][2],
                     "grad_logits": eager[1], "grad_baseline": eager[2]}
            pg_abs = R.impala_pg_abs(c["logits"], c["actions"], c["pg_adv"])
            for name in LOSS_NAMES:
                bad += _recorded_bound(
                    LOSS_MEASURED, _loss_key(T, B, A, scale, ec), name, got[name].cpu(),
                    want[name], LOSS_ATOL[name],
                    (e_ref[name].double() - want[name]).abs().max().item(),
                    sum_scale=pg_abs if name == "pg" else None)
        assert not bad, bad

    def test_kernel_grad_scale(self):
        """An upstream gradient other than 1, in the kernel itself."""
        from moolib_amd import _kernels

        T, B, A = 3, 5, 6
        c = loss_case(T, B, A, 2.0)
        args = (c["logits"], c["actions"], c["pg_adv"], c["vs"], c["baseline"], 0.01, 0.5)
        ref = R.impala_loss_ref(*args, grad_scale=3.0)
        _, gl, gb = _kernels.impala_loss(*(t.cuda() for t in args[:5]), 0.01, 0.5, 3.0)
        bad = []
        for name, got, want in (("grad_logits", gl, ref[1]), ("grad_baseline", gb, ref[2])):
            bad += _recorded_bound(LOSS_MEASURED, ("grad_scale", 3.0), name, got.cpu(), want,
                                   LOSS_ATOL[name], None)
        assert not bad, bad

    @pytest.mark.parametrize("layout", ["contiguous_int32_actions", "transposed_logits"])
    def test_total_loss_autograd(self, layout):
        """fused_loss.impala_total_loss with (3*total).backward(): the upstream
        gradient reaches both gradients; int32 actions work as in the eager
        path; non-contiguous logits get their gradient in their own layout."""
        from moolib_amd.ops import fused_loss

        T, B, A = 3, 5, 6
        c = loss_case(T, B, A, 2.0, seed=1)
        args = (c["logits"], c["actions"], c["pg_adv"], c["vs"], c["baseline"], 0.01, 0.5)
        ref = R.impala_loss_ref(*args, grad_scale=3.0)
        if layout == "transposed_logits":
            leaf = c["logits"].transpose(0, 1).contiguous().cuda().requires_grad_()  # [B,T,A]
            logits = leaf.transpose(0, 1)
            assert not logits.is_contiguous()
            actions = c["actions"].cuda()
        else:
            leaf = logits = c["logits"].cuda().requires_grad_()
            actions = c["actions"].to(torch.int32).cuda()
        baseline = c["baseline"].cuda().requires_grad_()
        total = fused_loss.impala_total_loss(
            logits, baseline, actions, c["pg_adv"].cuda(), c["vs"].cuda(), 0.01, 0.5)
        (3.0 * total).backward()
        gl = leaf.grad.transpose(0, 1) if layout == "transposed_logits" else leaf.grad
        key = ("total", layout)
        pg_abs = R.impala_pg_abs(c["logits"], c["actions"], c["pg_adv"])
        bad = _recorded_bound(LOSS_MEASURED, key, "total", total.detach().cpu(), ref[0].sum(),
                              1e-4, None, sum_scale=pg_abs + ref[0][1:].abs().sum().item())
        bad += _recorded_bound(LOSS_MEASURED, key, "grad_logits", gl.cpu(), ref[1], 1e-5, None)
        bad += _recorded_bound(LOSS_MEASURED, key, "grad_baseline", baseline.grad.cpu(), ref[2],
                               1e-5, None)
        assert not bad, bad


@gpu
@requires_gpu
class TestVtraceFp64:
    @pytest.mark.parametrize("T,B", VTRACE_SHAPES)
    def test_clip_branches(self, T, B):
        from moolib_amd.ops import vtrace

        v = vtrace_case(T, B)
        bad = []
        for clips in VTRACE_CLIPS:
            ref = R.vtrace_ref(*v.values(), *clips)
            e32 = R.vtrace_ref(*v.values(), *clips, dtype=torch.float32)
            dev = vtrace.from_importance_weights(
                *(t.cuda() for t in v.values()), clip_rho_threshold=clips[0],
                clip_pg_rho_threshold=clips[1])
            key = (T, B, str(clips[0]), str(clips[1]))
            for name, got, want, e in (("vs", dev.vs, ref[0], e32[0]),
                                       ("pg_advantages", dev.pg_advantages, ref[1], e32[1])):
                bad += _recorded_bound(VTRACE_MEASURED, key, name, got.cpu(), want, 1e-4,
                                       (e.double() - want).abs().max().item())
        assert not bad, bad
        if T > 1:  # the thresholds are visibly different ops on these inputs
            a, b = (R.vtrace_ref(*v.values(), *c)[0] for c in VTRACE_CLIPS[:2])
            assert (a - b).abs().max() > 1e-2


@gpu
@requires_gpu
class TestLstmFp64:
    @pytest.mark.parametrize("T,B", LSTM_CASES)
    def test_forward_backward(self, T, B):
        """max|kernel - R_exact| <= 2*d + 2**-8 * max|R_exact| per tensor, with
        d = max|R_emul - R_exact| from the CPU alone; never looser than the
        older fp32-reference tolerance."""
        from moolib_amd.ops.lstm import fused_lstm_scan

        d, exact, emul = lstm_refs(T, B)
        X, h0 = (d[k].to(BF16).cuda().requires_grad_() for k in ("X", "h0"))
        # fp32 leaves (values are bf16-representable): dW arrives unrounded
        c0, w = (d[k].float().cuda().requires_grad_() for k in ("c0", "w"))
        H, hT, cT = fused_lstm_scan(X, d["nd"].float().cuda(), h0, c0, w)
        loss = ((H.float() * d["gH"].float().cuda()).sum()
                + (hT.float() * d["ghT"].float().cuda()).sum()
                + (cT * d["gcT"].float().cuda()).sum())
        loss.backward()
        got = {"H": H, "hT": hT, "cT": cT, "dX": X.grad, "dh0": h0.grad, "dc0": c0.grad,
               "dW": w.grad}
        bounds = R.lstm_bounds(exact, emul)
        failures = []
        for k in R.LSTM_TENSORS:
            err = (got[k].detach().cpu().double() - exact[k]).abs().max().item()
            dist, bound = bounds[k]
            atol, rel = LSTM_PRESENT[k]
            bound = min(bound, atol + rel * exact[k].abs().max().item())
            _figure(kind="lstm", case=[T, B], tensor=k, d=dist, err=err, bound=bound)
            if err > bound:
                failures.append((k, err, bound))
        assert not failures, failures


# ============================================================== host checks


@gpu
@requires_gpu
class TestHostChecks:
    """One rejected call per host-side check; none of them may reach a launch."""

    def _conv_args(self, C=16, K=16, epi=0):
        x = torch.zeros(1, C, 2, 3, dtype=BF16, device="cuda").contiguous(
            memory_format=torch.channels_last)
        wp = torch.zeros((9 * C + 31) // 32 * 32 * K, dtype=BF16, device="cuda")
        return x, wp

    def test_conv3x3_rejects(self):
        from moolib_amd import _kernels

        f = _kernels.conv3x3_nhwc_fused
        C = K = 16
        x, wp = self._conv_args()
        vec = lambda n, dt=BF16: torch.zeros(n, dtype=dt, device="cuda")
        res = torch.zeros(1, K, 2, 3, dtype=BF16, device="cuda").contiguous(
            memory_format=torch.channels_last)
        f(x, wp, K, True, vec(C), 3, vec(K), res, vec(K), 0)  # the accepted form
        bad = {
            "epi 3 without res": (x, wp, K, False, None, 3, vec(K), None, None, 0),
            "res of another shape": (x, wp, K, False, None, 3, vec(K), res[:, :, :1], None, 0),
            "res not channels_last": (x, wp, K, False, None, 3, vec(K),
                                      res.contiguous(memory_format=torch.contiguous_format), None, 0),
            "res fp32": (x, wp, K, False, None, 3, vec(K), res.float(), None, 0),
            "epi 1 without bias1": (x, wp, K, False, None, 1, None, None, None, 0),
            "bias_in length": (x, wp, K, True, vec(C - 8), 0, None, None, None, 0),
            "bias1 length": (x, wp, K, False, None, 1, vec(K - 1), None, None, 0),
            "bias2 length": (x, wp, K, False, None, 3, vec(K), res, vec(2 * K), 0),
            "bias1 fp32": (x, wp, K, False, None, 2, vec(K, torch.float32), None, None, 0),
            "w_packed size": (x, wp[:-32], K, False, None, 0, None, None, None, 0),
            "w_packed for another K": (x, wp, 32, False, None, 0, None, None, None, 0),
            "epi out of range": (x, wp, K, False, None, 4, vec(K), res, None, 0),
            "rt 3": (x, wp, K, False, None, 0, None, None, None, 3),
        }
        for why, args in bad.items():
            with pytest.raises(RuntimeError):
                f(*args)
                pytest.fail(why)

    def test_wgrad_rejects_rows_that_fit_no_slab(self):
        from moolib_amd import _kernels

        mk = lambda c: torch.zeros(1, c, 1, 192, dtype=BF16, device="cuda").contiguous(
            memory_format=torch.channels_last)
        with pytest.raises(RuntimeError, match="too wide"):
            _kernels.wgrad3x3_nhwc(mk(32), mk(32))

    def test_lstm_rejects(self):
        from moolib_amd import _kernels

        T, B = 2, 3
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda")
        X, nd, h0, c0 = z(T, B, 1024, dt=BF16), z(T, B), z(B, 256, dt=BF16), z(B, 256)
        wp = z(1024 * 256, dt=BF16)
        H, gates, cs, hT, cT = _kernels.lstm_fused_fwd(X, nd, h0, c0, wp)  # accepted
        bad_fwd = {
            "notdone B": (X, z(T, B + 1), h0, c0, wp),
            "notdone dtype": (X, z(T, B, dt=torch.float64), h0, c0, wp),
            "h0 dtype": (X, nd, z(B, 256), c0, wp),
            "h0 B": (X, nd, z(B - 1, 256, dt=BF16), c0, wp),
            "h0 not contiguous": (X, nd, z(256, B, dt=BF16).t(), c0, wp),
            "c0 dtype": (X, nd, h0, z(B, 256, dt=BF16), wp),
            "c0 shape": (X, nd, h0, z(B, 128), wp),
            "c0 on the CPU": (X, nd, h0, torch.zeros(B, 256), wp),
            "packed weight size": (X, nd, h0, c0, wp[:-8]),
            "packed weight dtype": (X, nd, h0, c0, z(1024 * 256)),
            "X not contiguous": (z(B, T, 1024, dt=BF16).transpose(0, 1), nd, h0, c0, wp),
        }
        for why, args in bad_fwd.items():
            with pytest.raises(RuntimeError):
                _kernels.lstm_fused_fwd(*args)
                pytest.fail(why)
        dH, dhT, dcT = z(T, B, 256, dt=BF16), z(B, 256, dt=BF16), z(B, 256)
        _kernels.lstm_fused_bwd(gates, cs, c0, nd, dH, dhT, dcT, wp)  # accepted
        _kernels.lstm_fused_bwd(gates, cs, c0, nd, dH, torch.Tensor(), torch.Tensor(), wp)
        bad_bwd = {
            "gates dtype": (gates.float(), cs, c0, nd, dH, dhT, dcT, wp),
            "cs T": (gates, cs[:1], c0, nd, dH, dhT, dcT, wp),
            "c0 B": (gates, cs, z(B - 1, 256), nd, dH, dhT, dcT, wp),
            "notdone shape": (gates, cs, c0, z(T + 1, B), dH, dhT, dcT, wp),
            "dH shape": (gates, cs, c0, nd, z(T, B, 128, dt=BF16), dhT, dcT, wp),
            "dH dtype": (gates, cs, c0, nd, z(T, B, 256), dhT, dcT, wp),
            "dhT dtype": (gates, cs, c0, nd, dH, z(B, 256), dcT, wp),
            "dcT shape": (gates, cs, c0, nd, dH, dhT, z(B + 1, 256), wp),
            "packed weight size": (gates, cs, c0, nd, dH, dhT, dcT, wp[:-8]),
        }
        for why, args in bad_bwd.items():
            with pytest.raises(RuntimeError):
                _kernels.lstm_fused_bwd(*args)
                pytest.fail(why)

    def test_impala_loss_rejects(self):
        from moolib_amd import _kernels

        T, B, A = 2, 3, 4
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device="cuda")
        ok = [z(T, B, A), z(T, B, dt=torch.int64), z(T, B), z(T, B), z(T, B)]
        _kernels.impala_loss(*ok, 0.01, 0.5, 1.0)  # accepted
        for i, name in ((1, "actions"), (2, "pg_advantages"), (3, "vs"), (4, "baseline")):
            args = list(ok)
            args[i] = args[i][:, :-1]
            with pytest.raises(RuntimeError, match=name):
                _kernels.impala_loss(*args, 0.01, 0.5, 1.0)
        args = list(ok)
        args[1] = args[1].to(torch.int32)
        with pytest.raises(RuntimeError):
            _kernels.impala_loss(*args, 0.01, 0.5, 1.0)
