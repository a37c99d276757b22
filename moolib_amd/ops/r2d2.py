"""R2D2 loss (Kapturowski et al. 2019): n-step double-Q targets under the
invertible value rescaling h, masked sequence loss, mixed max/mean sequence
priorities.

All tensors are time-major: T network steps, B sequences, A actions.

    h(x)    = sign(x)(sqrt(|x|+1) - 1) + eps x
    a*_s    = argmax_a q[s,b,a]                       (lowest index wins ties)
    boot_s  = h^-1(q_target[s,b,a*_s])
    G_t     = sum_{i<k} (prod_{j<i} g_{t+j}) r_{t+i} + (prod_{j<k} g_{t+j}) boot_{t+k},
              k = min(n, T-1-t)                       (t < T-1)
    delta_t = valid_t (h(G_t) - q[t,b,a_t]),  valid_t = mask_t for t < T-1, 0 at T-1
    loss_seq[b] = 1/2 sum_t delta_t^2
    priority[b] = eta max_t|delta_t| + (1-eta) sum_t|delta_t| / max(1, sum_t valid_t)
    loss        = mean_b is_weights[b] loss_seq[b]

`discounts[t]` multiplies whatever follows step t and is 0 where the episode
ended after t (the convention of ops/vtrace.py); `rewards[t]` follows
`actions[t]`.

On an MI355X the whole loss, its analytic gradient w.r.t. q and the
priorities are one fused HIP kernel (moolib_amd._kernels.r2d2_loss);
autograd sees a single Function whose backward scales the precomputed
gradient. The plain-torch path below is the CPU implementation and the fp32
numerics reference of the kernel tests: it performs the same operations in
the same order.

`actor_priorities` is the actor's side of the same quantity: the initial
priority of a freshly acted sequence from the Q-values the act head returned
(q_taken, q_max), with reward and done in the actor's layout. One launch of
moolib_amd._kernels.r2d2_actor_priority on the GPU.
"""
import collections
import os

import torch

# Longest sequence the fused kernel takes (one thread per step, the column in
# LDS); _kernels.R2D2_MAX_T is the same number. Longer sequences are rejected
# on the GPU path, not silently rerouted.
KERNEL_MAX_T = 256

R2D2LossReturns = collections.namedtuple(
    "R2D2LossReturns", ["loss", "td_errors", "priorities", "loss_per_sequence"]
)


def value_rescale(x, eps=1e-3):
    """h(x) = sign(x)(sqrt(|x|+1) - 1) + eps x."""
    return torch.sign(x) * (torch.sqrt(x.abs() + 1) - 1) + eps * x


def inverse_value_rescale(x, eps=1e-3):
    """h^-1 in the cancellation-free form: with a = |x|+1+eps and
    s = 2a / (sqrt(1 + 4 eps a) + 1), h^-1(x) = sign(x)(s^2 - 1). (The
    textbook ((sqrt(1+4 eps a) - 1) / (2 eps))^2 - 1 subtracts two nearly
    equal numbers and loses ~100x in fp32; it also divides by eps.)"""
    a = x.abs() + 1 + eps
    s = (2 * a) / (torch.sqrt(1 + (4 * eps) * a) + 1)
    return torch.sign(x) * (s * s - 1)


def dueling_q(value, advantage):
    """Q = V + A - mean_a A, value [...], advantage [..., A]."""
    return value.unsqueeze(-1) + advantage - advantage.mean(dim=-1, keepdim=True)


def _kernels():
    """The kernel module for a GPU call, or None if the eager path was asked
    for. A build without the kernels is an error on the GPU, not a quiet
    detour through ~100 eager launches."""
    if os.environ.get("MOOLIB_AMD_NO_R2D2_KERNEL"):
        return None
    try:
        from moolib_amd import _kernels as k
    except ImportError as e:
        raise ImportError(
            "r2d2_loss on a GPU tensor needs moolib_amd._kernels (python setup.py build_ext "
            "--inplace); set MOOLIB_AMD_NO_R2D2_KERNEL=1 to run the eager path instead"
        ) from e
    return k


@torch.no_grad()
def _rescaled_returns(q, q_target, rewards, discounts, n_step, eps, rescale):
    """h(G_t) for t < T-1: [T-1, B]. No gradient flows into the target."""
    a_star = q.argmax(dim=-1, keepdim=True)  # first maximal index
    boot = q_target.gather(-1, a_star).squeeze(-1)
    return _returns_from_bootstrap(boot, rewards, discounts, n_step, eps, rescale)


@torch.no_grad()
def _returns_from_bootstrap(boot, rewards, discounts, n_step, eps, rescale):
    """h(G_t) for t < T-1 from the value [T, B] each step bootstraps with."""
    T = boot.shape[0]
    if rescale:
        boot = inverse_value_rescale(boot, eps)
    Tm = T - 1
    G = torch.zeros_like(rewards[:Tm])
    disc = torch.ones_like(G)
    for i in range(min(n_step, Tm)):
        # steps whose window still holds reward t+i: t+i <= T-2
        m = Tm - i
        G[:m] += disc[:m] * rewards[i:Tm]
        disc[:m] *= discounts[i:Tm]
    boot_index = (torch.arange(Tm, device=boot.device) + n_step).clamp(max=T - 1)
    G += disc * boot[boot_index]
    if rescale:
        G = value_rescale(G, eps)
    return G


def _eager(q, q_target, actions, rewards, discounts, mask, is_weights, n_step, eps, rescale, eta):
    qa = q.gather(-1, actions.unsqueeze(-1)).squeeze(-1)
    G = _rescaled_returns(q.detach(), q_target.detach(), rewards, discounts, n_step, eps, rescale)
    valid = torch.cat([mask[:-1], torch.zeros_like(mask[-1:])], dim=0)
    td = torch.cat([mask[:-1] * (G - qa[:-1]), torch.zeros_like(qa[-1:])], dim=0)
    loss_seq = 0.5 * (td * td).sum(dim=0)
    with torch.no_grad():
        abs_td = td.abs()
        mean_abs = abs_td.sum(dim=0) / valid.sum(dim=0).clamp(min=1.0)
        priorities = eta * abs_td.max(dim=0).values + (1.0 - eta) * mean_abs
    loss = (is_weights * loss_seq).mean()
    return R2D2LossReturns(loss, td.detach(), priorities, loss_seq.detach())


class _FusedR2D2Loss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, q_target, actions, rewards, discounts, mask, is_weights, n_step, eps,
                rescale, eta):
        B = q.shape[1]
        td, loss_seq, priorities, grad_q = _kernels().r2d2_loss(
            q, q_target, actions, rewards, discounts, mask, is_weights,
            n_step, eps, rescale, eta, 1.0 / B,
        )
        ctx.save_for_backward(grad_q)
        ctx.mark_non_differentiable(td, priorities, loss_seq)
        loss = (is_weights * loss_seq).mean()
        return loss, td, priorities, loss_seq

    @staticmethod
    def backward(ctx, grad_loss, *unused):
        (grad_q,) = ctx.saved_tensors
        return (grad_q * grad_loss,) + (None,) * 10


def r2d2_loss(q, q_target, actions, rewards, discounts, mask, is_weights,
              n_step=5, eps=1e-3, rescale=True, eta=0.9):
    """R2D2 loss of a batch of sequences.

    q [T,B,A] fp32 (online network, receives the gradient), q_target [T,B,A]
    fp32 (no gradient), actions [T,B] any integer dtype, rewards / discounts
    / mask [T,B] fp32 (mask is 0 on burn-in and padding steps), is_weights
    [B]. Inputs need not be contiguous. Returns R2D2LossReturns(loss,
    td_errors [T,B], priorities [B], loss_per_sequence [B]); only `loss`
    is differentiable. Uses the fused gfx950 kernel on GPU (sequences of up
    to KERNEL_MAX_T steps), eager torch on the CPU or with
    MOOLIB_AMD_NO_R2D2_KERNEL set.
    """
    n_step, eps, rescale, eta = int(n_step), float(eps), bool(rescale), float(eta)
    if n_step < 1:
        raise ValueError("r2d2_loss: n_step must be >= 1, got %d" % n_step)
    if eps < 0:
        raise ValueError("r2d2_loss: eps must be >= 0, got %r" % eps)
    if not 0.0 <= eta <= 1.0:
        raise ValueError("r2d2_loss: eta must be in [0,1], got %r" % eta)
    args = (
        q.float().contiguous(),
        q_target.detach().float().contiguous(),
        actions.to(torch.int64).contiguous(),
        rewards.detach().float().contiguous(),
        discounts.detach().float().contiguous(),
        mask.detach().float().contiguous(),
        is_weights.detach().float().contiguous(),
    )
    if q.is_cuda and _kernels() is not None:
        return R2D2LossReturns(*_FusedR2D2Loss.apply(*args, n_step, eps, rescale, eta))
    return _eager(*args, n_step, eps, rescale, eta)


ActorPriorityReturns = collections.namedtuple("ActorPriorityReturns", ["priorities", "td_errors"])


@torch.no_grad()
def _eager_actor_priorities(q_taken, q_max, reward, done, n_step, discount, eps, rescale, eta,
                            burn_in):
    T = q_taken.shape[0]
    # r_t and gamma_t FOLLOW a_t: they arrive with step t+1. The last step has
    # no successor; it only bootstraps.
    last = torch.zeros_like(reward[:1])
    rewards = torch.cat([reward[1:], last], dim=0)
    gamma = torch.full_like(reward[1:], discount)
    discounts = torch.cat([torch.where(done[1:] != 0, torch.zeros_like(gamma), gamma), last], dim=0)
    G = _returns_from_bootstrap(q_max, rewards, discounts, n_step, eps, rescale)
    valid = torch.zeros_like(reward)
    valid[burn_in:T - 1] = 1.0
    td = torch.cat([valid[:-1] * (G - q_taken[:-1]), last], dim=0)
    abs_td = td.abs()
    mean_abs = abs_td.sum(dim=0) / valid.sum(dim=0).clamp(min=1.0)
    priorities = eta * abs_td.max(dim=0).values + (1.0 - eta) * mean_abs
    return ActorPriorityReturns(priorities, td)


def actor_priorities(q_taken, q_max, reward, done, *, n_step=5, discount=0.997, eps=1e-3,
                     rescale=True, eta=0.9, burn_in=0, out=None):
    """Initial replay priorities of an actor's sequences, from its own Q-values.

    q_taken / q_max [T,K] are the Q-values of the actions taken and of the
    greedy ones (R2D2Learner.act(..., return_q=True)); reward [T,K] and done
    [T,K] (bool or uint8) are in the actor's layout, as replay items hold them:
    reward[t] and done[t] arrive WITH step t, so they follow action t-1. The
    shift by one step happens in here:

        r_t = reward[t+1],  g_t = done[t+1] ? 0 : discount        (t < T-1)
        boot_s  = h^-1(q_max[s])
        G_t     = n-step return of r, g, boot as in r2d2_loss
        delta_t = valid_t (h(G_t) - q_taken[t]),  valid_t = 1 for burn_in <= t < T-1
        priority[k] = eta max_t|delta_t| + (1-eta) sum_t|delta_t| / max(1, sum_t valid_t)

    which is what r2d2_loss returns when the target network equals the online
    one. Rewards are not clipped. Returns ActorPriorityReturns(priorities [K],
    td_errors [T,K]). `out`, a (priorities, td_errors) pair of contiguous fp32
    buffers, receives the results. One launch of the fused gfx950 kernel on the
    GPU (T up to KERNEL_MAX_T, no host synchronisation), plain torch on the
    CPU or with MOOLIB_AMD_NO_R2D2_KERNEL set.
    """
    n_step, discount, eps = int(n_step), float(discount), float(eps)
    rescale, eta, burn_in = bool(rescale), float(eta), int(burn_in)
    if n_step < 1:
        raise ValueError("actor_priorities: n_step must be >= 1, got %d" % n_step)
    if eps < 0:
        raise ValueError("actor_priorities: eps must be >= 0, got %r" % eps)
    if not 0.0 <= eta <= 1.0:
        raise ValueError("actor_priorities: eta must be in [0,1], got %r" % eta)
    if burn_in < 0:
        raise ValueError("actor_priorities: burn_in must be >= 0, got %d" % burn_in)
    if q_taken.dim() != 2 or q_taken.shape[0] < 1:
        raise ValueError("actor_priorities: q_taken must be [T,K] with T >= 1, got %s"
                         % (tuple(q_taken.shape),))
    for name, t in (("q_max", q_max), ("reward", reward), ("done", done)):
        if t.shape != q_taken.shape:
            raise ValueError("actor_priorities: %s has shape %s, q_taken %s"
                             % (name, tuple(t.shape), tuple(q_taken.shape)))
        if t.device != q_taken.device:
            raise ValueError("actor_priorities: %s is on %s, q_taken on %s"
                             % (name, t.device, q_taken.device))
    if done.dtype not in (torch.bool, torch.uint8):
        done = done != 0
    args = (
        q_taken.detach().float().contiguous(),
        q_max.detach().float().contiguous(),
        reward.detach().float().contiguous(),
        done.contiguous(),
    )
    if q_taken.is_cuda and _kernels() is not None:
        priority_out, td_out = out if out is not None else (None, None)
        return ActorPriorityReturns(*_kernels().r2d2_actor_priority(
            *args, n_step, discount, eps, rescale, eta, burn_in, priority_out, td_out))
    result = _eager_actor_priorities(*args, n_step, discount, eps, rescale, eta, burn_in)
    if out is not None:
        out[0].copy_(result.priorities)
        out[1].copy_(result.td_errors)
        return ActorPriorityReturns(out[0], out[1])
    return result
