"""The policy and baseline heads as one op (hip/heads.hip.inc): one MFMA launch
forward, two backward, fp32 outputs straight from the fp32 accumulators.

Dense mode (models with an LSTM), x [M, D], D in (128, 256, 512):

    logits[m, a] = sum_k x[m, k] * bf16(Wp[a, k]) + bp[a]
    baseline[m]  = sum_k x[m, k] * bf16(Wb[0, k]) + bb[0]

Composite mode (models without one), x [M, 256] = relu(fc), weights [., 257+A]
in the model's column order (features, reward, actions):

    logits[m, a] = sum_{k<256} x[m, k] * bf16(Wp[a, k])
                   + clamp(reward[m], -1, 1) * bf16(Wp[a, 256])
                   + bf16(Wp[a, 257 + p_m]) + bp[a]

and the same form for the baseline: no one_hot, clamp or cat, and the reward
stays fp32. The weights and biases are `nn.Linear`'s own tensors, fp32 or bf16,
read where they lie (no cast copy under autocast, no transpose, no pack, no cat
of the two heads). No atomics, no host sync, graph-capturable.
"""
import torch
import torch.nn.functional as F

HEADS_WIDTHS = (128, 256, 512)
HEADS_COMPOSITE_WIDTH = 256
HEADS_MAX_ACTIONS = 63


def _kernels():
    try:
        from moolib_amd import _kernels as k

        return k
    except ImportError:
        return None


def heads_available(width, num_actions, composite, device):
    """Whether policy_value_heads runs its kernels for this shape on `device`."""
    return (
        (width == HEADS_COMPOSITE_WIDTH if composite else width in HEADS_WIDTHS)
        and 1 <= num_actions <= HEADS_MAX_ACTIONS
        and device.type == "cuda"
        and _kernels() is not None
    )


def heads_eager(x, policy_weight, policy_bias, baseline_weight, baseline_bias,
                reward=None, prev_action=None):
    """The same math in plain torch, in x's dtype, outputs .float(): what
    AtariNet computes without the op (one_hot, clamp, cat in composite mode,
    then the two F.linear). An action outside [0, A) gives an all-zero one-hot
    row."""
    if (reward is None) != (prev_action is None):
        raise ValueError("heads: reward and prev_action come together or not at all")
    if reward is not None:
        A = policy_weight.shape[0]
        action = prev_action.reshape(-1).to(torch.int64)
        valid = ((action >= 0) & (action < A)).unsqueeze(-1)
        onehot = F.one_hot(action.clamp(0, A - 1), A).to(x.dtype) * valid.to(x.dtype)
        clipped = reward.reshape(-1, 1).clamp(-1, 1).to(x.dtype)
        x = torch.cat([x, clipped, onehot], dim=-1)
    logits = F.linear(x, policy_weight.to(x.dtype), policy_bias.to(x.dtype)).float()
    baseline = F.linear(x, baseline_weight.to(x.dtype), baseline_bias.to(x.dtype)).float()
    return logits, baseline.reshape(-1)


class _Heads(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pw, pb, bw, bb, reward, prev_action):
        logits, baseline = _kernels().heads_fwd(x, pw, pb, bw, bb, reward, prev_action)
        ctx.save_for_backward(x, pw, bw, reward, prev_action)
        ctx.set_materialize_grads(False)  # an unused output's gradient arrives as None
        return logits, baseline

    @staticmethod
    def backward(ctx, dlogits, dbaseline):
        x, pw, bw, reward, prev_action = ctx.saved_tensors
        # the incoming fp32 gradients are read as they are; None counts as zero
        if dlogits is not None:
            dlogits = dlogits.float().contiguous()
        if dbaseline is not None:
            dbaseline = dbaseline.float().contiguous()
        dx, dpw, dpb, dbw, dbb = _kernels().heads_bwd(
            dlogits, dbaseline, x, pw, bw, reward, prev_action, ctx.needs_input_grad[0]
        )
        # the parameter gradients are fp32; autograd casts them for bf16 parameters
        return dx, dpw, dpb, dbw, dbb, None, None


def policy_value_heads(x, policy_weight, policy_bias, baseline_weight, baseline_bias,
                       reward=None, prev_action=None):
    """x [M, D]; policy_weight [A, K], policy_bias [A], baseline_weight [1, K],
    baseline_bias [1] (nn.Linear's). Dense mode: K = D in (128, 256, 512),
    reward and prev_action None. Composite mode: D = 256, K = 257 + A, reward
    [M] (not clipped, any real dtype) and prev_action [M] (any integer dtype).
    Returns (logits [M, A] fp32, baseline [M] fp32), see the module docstring.

    On a GPU with _kernels built this is one launch (two more in the backward):
    x bf16, weights fp32 or bf16 and rounded to bf16 as they are read, fp32
    accumulation, the fp32 result written directly. 1 <= A <= 63. Gradients: x
    bf16, the four parameters fp32 in their own layouts, none for reward and
    prev_action; either incoming gradient may be None; summed in a fixed order.
    An action outside [0, A) contributes nothing. Under no_grad, or when nothing
    requires a gradient, nothing is saved. Anything else on a GPU raises
    ValueError. On the CPU, or without _kernels, heads_eager runs."""
    if not x.is_cuda or _kernels() is None:
        return heads_eager(x, policy_weight, policy_bias, baseline_weight, baseline_bias,
                           reward, prev_action)
    served = ("served: x bf16 [M, D] with D in %s and weights [A, D], [1, D]; or with reward and "
              "prev_action [M], x [M, %d] and weights [A, %d+A], [1, %d+A]; 1 <= A <= %d; "
              "contiguous weights of one dtype, fp32 or bf16"
              % (HEADS_WIDTHS, HEADS_COMPOSITE_WIDTH, HEADS_COMPOSITE_WIDTH + 1,
                 HEADS_COMPOSITE_WIDTH + 1, HEADS_MAX_ACTIONS))
    if (reward is None) != (prev_action is None):
        raise ValueError("heads: reward and prev_action come together or not at all; " + served)
    composite = reward is not None
    if x.dim() != 2 or policy_weight.dim() != 2 or baseline_weight.dim() != 2:
        raise ValueError("heads: 2-d x and weights expected; " + served)
    A, K = policy_weight.shape
    D = x.shape[1]
    if (
        not heads_available(D, A, composite, x.device)
        or K != (D + 1 + A if composite else D)
        or tuple(baseline_weight.shape) != (1, K)
        or tuple(policy_bias.shape) != (A,)
        or tuple(baseline_bias.shape) != (1,)
    ):
        raise ValueError(
            "heads: no kernel for x %s, policy weight %s, baseline weight %s, %s reward; %s"
            % (tuple(x.shape), tuple(policy_weight.shape), tuple(baseline_weight.shape),
               "with" if composite else "without", served)
        )
    if x.dtype != torch.bfloat16:
        raise ValueError("heads: x must be bf16 on the GPU, got %s; %s" % (x.dtype, served))
    if policy_weight.dtype != baseline_weight.dtype or policy_weight.dtype not in (
        torch.float32, torch.bfloat16
    ):
        raise ValueError("heads: weights %s and %s; %s"
                         % (policy_weight.dtype, baseline_weight.dtype, served))
    if not (policy_weight.is_contiguous() and baseline_weight.is_contiguous()):
        raise ValueError("heads: the weights must be contiguous; " + served)
    if composite:
        reward, prev_action = reward.reshape(-1).contiguous(), prev_action.reshape(-1).contiguous()
        if reward.shape[0] != x.shape[0] or prev_action.shape[0] != x.shape[0]:
            raise ValueError("heads: reward and prev_action must have M = %d elements" % x.shape[0])
    args = (x.contiguous(), policy_weight, policy_bias.contiguous(), baseline_weight,
            baseline_bias.to(policy_bias.dtype).contiguous(), reward, prev_action)
    if torch.is_grad_enabled() and any(t.requires_grad for t in args[:5]):
        return _Heads.apply(*args)
    return tuple(_kernels().heads_fwd(*args))
