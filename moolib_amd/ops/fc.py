"""The trunk's FC layer as one op (hip/fc.hip.inc): the conv trunk's NHWC
features through relu(fc), forward and backward, on MFMA.

    feat[m, n] = relu( sum_{c,p} r(x[m, c, p]) * W[n, c*P + p] + b[n] )
    r = relu if relu_in else identity

`x` [M, 32, Hh, Ww] stays channels_last (no layout copy to the NCHW flatten and
none back in the backward), `W` is nn.Linear's own [256, 32*Hh*Ww] weight in its
own column order, fp32 or bf16, read where it lies (no cast copy under
autocast, no packed copy, so nothing can go stale after an optimizer step).
The forward splits the long reduction over workgroups and sums the partials in
a fixed order; the backward applies the fc relu's mask as the upstream gradient
is fetched and the trunk relu's mask in the input gradient's epilogue. No
atomics, no host sync, graph-capturable.
"""
import torch
import torch.nn.functional as F

TRUNK_FC_CHANNELS = 32
TRUNK_FC_WIDTH = 256


def _kernels():
    try:
        from moolib_amd import _kernels as k

        return k
    except ImportError:
        return None


def trunk_fc_available(C, device):
    """Whether trunk_fc runs its kernels for C channels on `device`."""
    return C == TRUNK_FC_CHANNELS and device.type == "cuda" and _kernels() is not None


def trunk_fc_eager(x, weight, bias, relu_in=False):
    """The definition in plain torch, in x's dtype, for any layout of x: the
    NCHW flatten (reshape of a channels_last tensor copies to that order),
    F.linear, relu."""
    if relu_in:
        x = F.relu(x)
    return F.relu(F.linear(x.reshape(x.shape[0], -1), weight.to(x.dtype), bias.to(x.dtype)))


class _TrunkFC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, relu_in, split_k):
        feat = _kernels().trunk_fc_fwd(x, weight, bias, relu_in, split_k)
        ctx.save_for_backward(x, weight, feat)
        ctx.relu_in = relu_in
        return feat

    @staticmethod
    def backward(ctx, dY):
        x, weight, feat = ctx.saved_tensors
        dx, dW, db = _kernels().trunk_fc_bwd(
            dY.contiguous(), x, feat, weight, ctx.relu_in, ctx.needs_input_grad[0]
        )
        # dW and db are fp32; autograd casts them to the parameters' dtype
        return dx, dW, db, None, None


def trunk_fc(x, weight, bias, relu_in=False, split_k=None):
    """x [M, 32, Hh, Ww]; weight [256, 32*Hh*Ww] (nn.Linear's, NCHW column
    order); bias [256]. Returns feat [M, 256] = relu(fc(flatten(r(x)))) with
    r = relu if `relu_in`.

    On a GPU with _kernels built: x bf16, made channels_last-dense if it is
    not; weight fp32 or bf16, rounded to bf16 as it is read; fp32 accumulation,
    bias and relu in fp32, one rounding to the bf16 result. One launch, or two
    when the reduction is split: `split_k` None lets (M, Hh*Ww) decide, 1 asks
    for a single pass, S > 1 for S slabs of pixels (clamped to Hh*Ww).
    Gradients: x bf16 channels_last (zero where x <= 0 when `relu_in`), weight
    and bias fp32, summed in a fixed order. C != 32, a weight that is not
    [256, 32*Hh*Ww] contiguous or a non-bf16 x raise ValueError.
    On the CPU, or without _kernels, trunk_fc_eager runs."""
    if not x.is_cuda or _kernels() is None:
        return trunk_fc_eager(x, weight, bias, relu_in)
    if x.dim() != 4 or not trunk_fc_available(x.shape[1], x.device):
        raise ValueError("trunk_fc: x [M,32,Hh,Ww] expected, got %s" % (tuple(x.shape),))
    if x.dtype != torch.bfloat16:
        raise ValueError("trunk_fc: x must be bf16 on the GPU, got %s" % x.dtype)
    K = x.shape[1] * x.shape[2] * x.shape[3]
    if tuple(weight.shape) != (TRUNK_FC_WIDTH, K) or not weight.is_contiguous():
        raise ValueError(
            "trunk_fc: weight must be [%d, %d] contiguous, got %s with strides %s"
            % (TRUNK_FC_WIDTH, K, tuple(weight.shape), tuple(weight.stride()))
        )
    if tuple(bias.shape) != (TRUNK_FC_WIDTH,):
        raise ValueError("trunk_fc: bias must be [%d], got %s" % (TRUNK_FC_WIDTH, tuple(bias.shape)))
    if split_k is not None and split_k < 1:
        raise ValueError("trunk_fc: split_k must be None or >= 1, got %r" % (split_k,))
    x = x.contiguous(memory_format=torch.channels_last)
    return _TrunkFC.apply(x, weight, bias.contiguous(), bool(relu_in),
                          0 if split_k is None else int(split_k))
