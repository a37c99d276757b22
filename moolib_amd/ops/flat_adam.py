"""Fused Adam step over flat buffers: gradient norm, clipping, update and the
bf16 shadow weights of all parameters at once.

`p`, `g`, `m`, `v` are flat fp32 buffers of N elements (every parameter, its
gradient and its two moments, laid out as moolib_amd.impala.
flatten_master_shadow does), `shadow` an optional flat bf16 buffer of N
elements, `step` a device int64 scalar counting the steps taken so far and
`lr` a device fp32 scalar. One call computes

    S    = sum_i (double) g_i * g_i,   norm = (float) sqrt(S)      (IEEE double sqrt)
    t    = step + 1
    coef = 1                                    if max_norm is None
    coef = min(1.0f, max_norm / (norm + 1e-6f)) otherwise (fp32)
    ĝ  = g * coef
    m' = m + (ĝ - m) * (1 - β1)
    v' = v * β2 + (1 - β2) * ĝ * ĝ
    p' = p - (lr / (1 - β1^t)) * m' / (sqrt(v') / sqrt(1 - β2^t) + eps)

writes `p'`, `m'`, `v'` in place, `shadow = bf16(p')` (round to nearest even,
NaN propagates), `step = t`, and returns `norm`, the unclipped gradient norm,
as a 0-dim fp32 tensor. `g` is left as it is (the clipped gradient is never
stored). These are `clip_grad_norm_`'s coefficient and `torch.optim.Adam`'s
update without weight decay, amsgrad or maximize.

Rounding: `1 - β1`, `1 - β2`, `1 - β1^t` and `1 - β2^t` are formed in double
and rounded to fp32 once; everything per element is fp32, IEEE `sqrt` and
division, no fused multiply-add, evaluated left to right as written:
`((1 - β2) * ĝ) * ĝ`, `((lr / bc1) * m') / (sqrt(v') / sqrt(bc2) + eps)`. A
NaN norm gives a NaN coefficient (`torch.clamp` keeps NaN), so a non-finite
gradient propagates as it does in torch; the step is not skipped.

On an MI355X this is two launches of hip/optim.hip.inc on the current stream
(`flat_sumsq`: per-block partial sums in double; `flat_adam_step`: every
block reduces the partials in the same fixed order, then updates its share),
with no atomics, no host wait and a grid that depends on N alone, so the
result is bit-reproducible. Elsewhere, or with MOOLIB_AMD_NO_FUSED_OPT set,
the plain-torch path below computes the same definition.
"""
import collections
import os

import torch

# Grid cap of the kernels and the number of elements one grid pass covers
# (1024 blocks x 256 threads x 4 elements); _kernels.FLAT_ADAM_MAX_BLOCKS and
# _kernels.FLAT_ADAM_PASS_ELEMENTS are the same numbers. PASS_ELEMENTS + 1 is
# the first N at which the grid-stride loop iterates.
MAX_BLOCKS = 1024
PASS_ELEMENTS = MAX_BLOCKS * 256 * 4

# What a kernel call needs besides its operands: the per-block partial sums of
# the norm, the second word of the step counter (no kernel reads and writes the
# same one) and the norm itself. FlatAdam keeps one, so a step allocates
# nothing.
Workspace = collections.namedtuple("Workspace", ["partial", "step_next", "norm"])


def new_workspace(device):
    return Workspace(
        torch.zeros(MAX_BLOCKS, dtype=torch.float64, device=device),
        torch.zeros((), dtype=torch.int64, device=device),
        torch.zeros((), dtype=torch.float32, device=device),
    )


def _kernels():
    """The kernel module for a GPU call, or None if the eager path was asked
    for. A build without the kernels is an error on the GPU, not a quiet
    detour through the eager launch chain."""
    if os.environ.get("MOOLIB_AMD_NO_FUSED_OPT"):
        return None
    try:
        from moolib_amd import _kernels as k
    except ImportError as e:
        raise ImportError(
            "flat_adam_step on a GPU tensor needs moolib_amd._kernels (python setup.py build_ext "
            "--inplace); set MOOLIB_AMD_NO_FUSED_OPT=1 to run the eager path instead"
        ) from e
    return k


def _check(p, g, m, v, step, lr, beta1, beta2, eps, shadow, max_norm):
    for name, t in (("p", p), ("g", g), ("m", m), ("v", v)):
        if t.dtype != torch.float32 or t.dim() != 1 or not t.is_contiguous():
            raise ValueError("flat_adam_step: %s must be a contiguous 1-D float32 tensor" % name)
        if t.numel() != p.numel() or t.device != p.device:
            raise ValueError(
                "flat_adam_step: %s must have p's length (%d) and device" % (name, p.numel())
            )
        if t.data_ptr() % 16:
            raise ValueError("flat_adam_step: %s must be 16-byte aligned" % name)
    if p.numel() < 1:
        raise ValueError("flat_adam_step: p must hold at least one element")
    if shadow is not None:
        if (shadow.dtype != torch.bfloat16 or shadow.dim() != 1 or not shadow.is_contiguous()
                or shadow.numel() != p.numel() or shadow.device != p.device):
            raise ValueError(
                "flat_adam_step: shadow must be a contiguous 1-D bfloat16 tensor of p's length "
                "and device"
            )
        if shadow.data_ptr() % 8:
            raise ValueError("flat_adam_step: shadow must be 8-byte aligned")
    if step.dtype != torch.int64 or step.numel() != 1 or step.device != p.device:
        raise ValueError("flat_adam_step: step must be one int64 element on p's device")
    if lr.dtype != torch.float32 or lr.numel() != 1 or lr.device != p.device:
        raise ValueError("flat_adam_step: lr must be one float32 element on p's device")
    if not (0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0):
        raise ValueError("flat_adam_step: betas must be in [0,1), got %r" % ((beta1, beta2),))
    if not eps >= 0.0:
        raise ValueError("flat_adam_step: eps must be >= 0, got %r" % eps)
    if max_norm is not None and not max_norm > 0.0:
        raise ValueError("flat_adam_step: max_norm must be > 0 or None, got %r" % max_norm)


@torch.no_grad()
def _eager(p, g, m, v, step, lr, beta1, beta2, eps, shadow, max_norm):
    g64 = g.double()
    norm = (g64 * g64).sum().sqrt().float()
    t = (step + 1).reshape(())
    lr = lr.reshape(())
    gh = g
    if max_norm is not None:
        coef = torch.full((), max_norm, dtype=torch.float32, device=g.device) / (norm + 1e-6)
        gh = g * torch.clamp(coef, max=1.0)
    m.add_((gh - m) * (1.0 - beta1))
    v.mul_(beta2).add_((gh * (1.0 - beta2)) * gh)
    t64 = t.double()
    one = torch.ones((), dtype=torch.float64, device=g.device)
    bc1 = (one - torch.pow(one * beta1, t64)).float()
    bc2 = (one - torch.pow(one * beta2, t64)).float()
    denom = v.sqrt() / bc2.sqrt() + eps
    p.sub_(((lr / bc1) * m) / denom)
    if shadow is not None:
        shadow.copy_(p)
    step.copy_(t.reshape(step.shape))
    return norm


def flat_adam_step(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, shadow=None,
                   max_norm=None, workspace=None):
    """One Adam step over flat buffers (see the module docstring).

    p, g, m, v: 1-D contiguous fp32 of equal length N >= 1 on one device,
    16-byte aligned; shadow: None or bf16 of length N, 8-byte aligned; step:
    one int64 element, lr: one fp32 element, both on that device; betas in
    [0, 1), eps >= 0, max_norm > 0 or None. Returns the unclipped gradient
    norm (0-dim fp32) without waiting for the device. With a `workspace`
    (see `new_workspace`) the GPU path allocates nothing and the returned norm
    is the workspace's own tensor, overwritten by the next call.
    """
    beta1, beta2, eps = float(beta1), float(beta2), float(eps)
    max_norm = None if max_norm is None else float(max_norm)
    _check(p, g, m, v, step, lr, beta1, beta2, eps, shadow, max_norm)
    k = _kernels() if p.is_cuda else None
    if k is None:
        return _eager(p, g, m, v, step, lr, beta1, beta2, eps, shadow, max_norm)
    ws = workspace if workspace is not None else new_workspace(p.device)
    k.flat_adam_step(p, g, m, v, shadow, step, ws.step_next, lr, ws.partial, ws.norm,
                     beta1, beta2, eps, max_norm)
    return ws.norm
