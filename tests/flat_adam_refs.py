"""float64 reference and input generators for the fused flat Adam step
(docs/KERNEL_TESTS.md, "Optimizer"). Written from the definition

    S = sum g^2, norm = sqrt(S), t = step + 1
    coef = 1 if max_norm is None else min(1.0f, max_norm / (norm + 1e-6f))   (fp32)
    gh = g coef
    m' = m + (gh - m)(1 - b1)
    v' = v b2 + (1 - b2) gh gh
    p' = p - (lr / (1 - b1^t)) m' / (sqrt(v') / sqrt(1 - b2^t) + eps)

not from moolib_amd/ops/flat_adam.py. A plain helper module (like
kernel_refs.py), used by tests/test_flat_adam.py.
"""
import collections
import functools

import numpy as np
import torch

Step = collections.namedtuple("Step", ["p", "m", "v", "norm", "t", "coef"])


def clip_coef(norm64, max_norm, fp32=True):
    """The definition forms the coefficient in fp32 from the fp32 norm; with
    fp32=False it is the same expression in float64 (what clip_grad_norm_
    computes on float64 gradients)."""
    if max_norm is None:
        return 1.0
    if fp32:
        n = np.float32(norm64)
        c = np.float32(max_norm) / (n + np.float32(1e-6))
        return float(min(np.float32(1.0), c))
    return min(1.0, max_norm / (norm64 + 1e-6))


def flat_adam_ref(p, g, m, v, step, lr, beta1, beta2, eps, max_norm=None, coef_fp32=True):
    """One step on float64 tensors (inputs untouched). `step` is the number of
    steps taken before this one."""
    p, g, m, v = (x.detach().double() for x in (p, g, m, v))
    norm = float((g * g).sum().sqrt())
    t = int(step) + 1
    coef = clip_coef(norm, max_norm, coef_fp32)
    gh = g * coef
    m1 = m + (gh - m) * (1.0 - beta1)
    v1 = v * beta2 + (1.0 - beta2) * gh * gh
    bc1 = 1.0 - beta1 ** t
    bc2 = 1.0 - beta2 ** t
    p1 = p - (lr / bc1) * m1 / (v1.sqrt() / np.sqrt(bc2) + eps)
    return Step(p1, m1, v1, norm, t, coef)


# ------------------------------------------------------------ integer-exact

INT = dict(beta1=0.5, beta2=0.75, eps=1.0, lr=2.0 ** -3)
INT_CLIP_MIN_N = 144  # 84 + 50 + 10 non-zero gradients
INT_VALUES = (0.0, 1.0, -1.0, 3.0, -3.0, 7.0, -7.0)


@functools.lru_cache(maxsize=None)
def integer_case(N, kind):
    """fp32 (p, g, max_norm) for step 0 -> 1 with m = v = 0.

    kind "none":   gradients in {0, +-1, +-3, +-7}, no clipping.
    kind "clamp":  the same gradients, max_norm = 2^20: the coefficient clamps to 1.
    kind "clip":   exactly 84 values +-2, 50 values +-6, 10 values +-14 at
                   random positions, 0 elsewhere: S = 4096, norm = 64, and in
                   fp32 64 + 1e-6 == 64, so max_norm = 32 gives coef = 0.5
                   and clipped gradients in {0, +-1, +-3, +-7}. Needs N >= 144.
    """
    gen = torch.Generator().manual_seed(1000003 * {"none": 1, "clamp": 2, "clip": 3}[kind] + N)
    p = torch.randint(-8, 9, (N,), generator=gen).float()
    if kind == "clip":
        assert N >= INT_CLIP_MIN_N
        mags = torch.cat([torch.full((84,), 2.0), torch.full((50,), 6.0), torch.full((10,), 14.0)])
        signs = torch.randint(0, 2, (144,), generator=gen).float() * 2 - 1
        g = torch.zeros(N)
        g[torch.randperm(N, generator=gen)[:144]] = mags * signs
        return p, g, 32.0
    # +-7 moves p by 7/64, which bf16 cannot hold next to |p| >= 4: weighting
    # it makes ties and inexact shadow values common
    vals = torch.tensor(INT_VALUES)
    weights = torch.tensor([0.1, 0.05, 0.05, 0.1, 0.1, 0.3, 0.3])
    g = vals[torch.multinomial(weights, N, replacement=True, generator=gen)]
    return p, g, (None if kind == "none" else 2.0 ** 20)


@functools.lru_cache(maxsize=None)
def integer_ref(N, kind):
    p, g, max_norm = integer_case(N, kind)
    z = torch.zeros(N)
    return flat_adam_ref(p, g, z, z, 0, INT["lr"], INT["beta1"], INT["beta2"], INT["eps"], max_norm)


# -------------------------------------------------------------------- float

FLOAT = dict(lr=6e-4, beta1=0.9, beta2=0.999)
FLOAT_SCALES = (1e-3, 1.0, 1e3)
FLOAT_EPS = (1e-8, 1e-3)
FLOAT_MAX_NORM = (None, 40.0, 1e-2)
FLOAT_STEP = 3  # m and v come from 3 earlier reference steps


@functools.lru_cache(maxsize=None)
def float_case(N, scale, eps, max_norm):
    """fp32 (p, g, m, v) at step 3: unit-normal p, gradients of `scale`, the
    moments of 3 earlier float64 reference steps rounded to fp32."""
    gen = torch.Generator().manual_seed(int(N) * 7 + int(np.log10(scale)) + 11)
    p = torch.randn(N, generator=gen, dtype=torch.float64)
    m = torch.zeros(N, dtype=torch.float64)
    v = torch.zeros(N, dtype=torch.float64)
    for s in range(FLOAT_STEP):
        g = scale * torch.randn(N, generator=gen, dtype=torch.float64)
        out = flat_adam_ref(p, g.float(), m, v, s, FLOAT["lr"], FLOAT["beta1"], FLOAT["beta2"],
                            eps, max_norm)
        p, m, v = out.p, out.m, out.v
    g = (scale * torch.randn(N, generator=gen, dtype=torch.float64)).float()
    return p.float(), g, m.float(), v.float()


@functools.lru_cache(maxsize=None)
def float_ref(N, scale, eps, max_norm):
    p, g, m, v = float_case(N, scale, eps, max_norm)
    return flat_adam_ref(p, g, m, v, FLOAT_STEP, FLOAT["lr"], FLOAT["beta1"], FLOAT["beta2"], eps,
                         max_norm)


def split_sizes(N, k):
    """N elements over k tensors, as evenly as they go (some may be empty)."""
    return [N // k + (1 if i < N % k else 0) for i in range(k)]
