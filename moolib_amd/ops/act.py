"""Fused actor head: counter-based action sampling and the epsilon-greedy
dueling head, each one launch, with no torch generator behind them.

Random numbers. The whole sampler state is two int64 on the device,
`[seed, step]`. A call reads `step`, draws from Philox4x32 with 10 rounds
(multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85)

    key     = (seed & 0xffffffff, seed >> 32)          seed taken as uint64
    counter = (row, 0, step & 0xffffffff, step >> 32)
    u0 = (x0 >> 8) * 2^-24,  u1 = (x1 >> 8) * 2^-24    exact float32 in [0, 1)

(x2, x3 unused) and stores `step + 1`. A captured launch therefore draws
fresh numbers on every replay, and any draw can be recomputed on the CPU from
(seed, step, row): `philox_uniforms`. With explicit uniforms `u` [N, 2] the
state is neither read nor advanced; that is the test hook and the definition
of the arithmetic below. Everything is fp32, sums strictly in order
a = 0..A-1, 1 <= A <= 64.

sample_categorical, per row of logits l:

    m      = max_a l_a
    e_a    = expf(l_a - m)
    total  = ((e_0 + e_1) + ...)
    target = u0 * total
    action = the first a whose running sum ((e_0 + e_1) + ... + e_a) > target,
             or, if there is none (rounding at the top), the last a with e_a > 0

An action of zero probability (e_a == 0, -inf logits included) is never
returned. (The scan repeats the additions of `total`, and fp32 u0 * total
stays below total for every u0 < 1, so the second case needs an explicit
u0 = 1; it is there so that no input can yield an action out of range.) Rows
that hold NaN or +inf are outside the contract.

epsilon_greedy_dueling, per row of (value v, advantage adv, epsilon):

    s      = ((adv_0 + adv_1) + ...)
    mean   = s / (float) A
    q_a    = (v + adv_a) - mean
    greedy = the lowest index of max_a q_a             (the tie rule of ops/r2d2.py)
    explore       = u0 < epsilon
    random_action = min(A - 1, (int) floorf(u1 * (float) A))
    action  = explore ? random_action : greedy
    q_taken = q[action],  q_max = q[greedy]

Every operation of the second is an exact integer or a single IEEE operation,
so CPU and GPU agree bit for bit; the first agrees wherever expf does.

On an MI355X each op is one launch of a HIP kernel of moolib_amd._kernels
(act_categorical, act_eps_greedy), and neither waits for the device. The
plain-torch path below is the CPU implementation and the fp32 reference of
the kernel tests: it performs the same operations in the same order.
"""
import os

import torch

# Widest row the kernels take (_kernels.ACT_MAX_ACTIONS is the same number);
# wider rows are rejected, not rerouted.
KERNEL_MAX_ACTIONS = 64

_M32 = 0xFFFFFFFF
_M64 = 0xFFFFFFFFFFFFFFFF
_PHILOX_M0 = 0xD2511F53
_PHILOX_M1 = 0xCD9E8D57
_PHILOX_W0 = 0x9E3779B9
_PHILOX_W1 = 0xBB67AE85


def _kernels():
    """The kernel module for a GPU call, or None if the eager path was asked
    for. A build without the kernels is an error on the GPU, not a quiet
    detour through eager launches."""
    if os.environ.get("MOOLIB_AMD_NO_ACT_KERNEL"):
        return None
    try:
        from moolib_amd import _kernels as k
    except ImportError as e:
        raise ImportError(
            "act ops on a GPU tensor need moolib_amd._kernels (python setup.py build_ext "
            "--inplace); set MOOLIB_AMD_NO_ACT_KERNEL=1 to run the eager path instead"
        ) from e
    return k


def new_state(seed, device="cpu"):
    """A sampler state `[seed, 0]`: int64 [2] on `device`. `seed` is any
    integer; it is taken modulo 2^64."""
    seed = int(seed) & _M64
    if seed >= 1 << 63:
        seed -= 1 << 64
    return torch.tensor([seed, 0], dtype=torch.int64, device=device)


def _mulhilo(m, x):
    """(high, low) 32-bit words of the product of the constant `m` < 2^32 and
    the int64 tensor `x` of values < 2^32, through 16-bit halves so that no
    intermediate leaves int64."""
    mh, ml = m >> 16, m & 0xFFFF
    xh, xl = x >> 16, x & 0xFFFF
    ll = xl * ml
    lh = xl * mh
    hl = xh * ml
    mid = (ll >> 16) + (lh & 0xFFFF) + (hl & 0xFFFF)
    lo = ((mid & 0xFFFF) << 16) | (ll & 0xFFFF)
    hi = xh * mh + (lh >> 16) + (hl >> 16) + (mid >> 16)
    return hi & _M32, lo


def _philox4x32(counter, key):
    """Philox4x32-10 of four int64 counter tensors (values < 2^32) under the
    key `(k0, k1)` of Python integers: the four output words, int64."""
    c0, c1, c2, c3 = counter
    k0, k1 = key[0] & _M32, key[1] & _M32
    for _ in range(10):
        hi0, lo0 = _mulhilo(_PHILOX_M0, c0)
        hi1, lo1 = _mulhilo(_PHILOX_M1, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = (k0 + _PHILOX_W0) & _M32
        k1 = (k1 + _PHILOX_W1) & _M32
    return c0, c1, c2, c3


def philox_uniforms(seed, step, n):
    """The uniforms (u0, u1) of rows 0..n-1 at `(seed, step)`: float32 [n, 2]
    on the CPU, computed with int64 arithmetic masked to 32 bits."""
    seed = int(seed) & _M64
    step = int(step) & _M64
    n = int(n)
    if not 1 <= n <= 1 << 31:
        raise ValueError("philox_uniforms: n must be in [1, 2^31], got %d" % n)
    row = torch.arange(n, dtype=torch.int64)
    zero = torch.zeros(n, dtype=torch.int64)
    x0, x1, _, _ = _philox4x32(
        (row, zero, zero + (step & _M32), zero + (step >> 32)), (seed & _M32, seed >> 32)
    )
    # 24 bits each: the conversion and the power-of-two scaling are exact
    return torch.stack([x0 >> 8, x1 >> 8], dim=1).to(torch.float32) * (2.0 ** -24)


def epsilon_ladder(n, base=0.4, alpha=7.0):
    """The Ape-X exploration schedule (Horgan et al. 2018): float32 [n],
    epsilon_i = base ** (1 + alpha * i / (n - 1)); n == 1 gives `base`."""
    n = int(n)
    if n < 1:
        raise ValueError("epsilon_ladder: n must be >= 1, got %d" % n)
    if n == 1:
        return torch.tensor([float(base)], dtype=torch.float32)
    i = torch.arange(n, dtype=torch.float64)
    return torch.pow(float(base), 1.0 + float(alpha) * i / (n - 1)).to(torch.float32)


def _rows(x, fn, name):
    """`x` [..., A] as contiguous float32 [N, A]."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
        raise ValueError("%s: %s must be a float32 tensor" % (fn, name))
    if x.dim() < 1 or x.numel() == 0:
        raise ValueError("%s: %s must be [..., A] with at least one row" % (fn, name))
    A = x.shape[-1]
    if not 1 <= A <= KERNEL_MAX_ACTIONS:
        raise ValueError(
            "%s: A must be in [1, %d], got %d" % (fn, KERNEL_MAX_ACTIONS, A)
        )
    return x.detach().reshape(-1, A).contiguous()


def _source(state, u, like, N, fn):
    """Checks that exactly one of `state` and `u` is given and well-formed;
    returns `u` as contiguous [N, 2] (or None)."""
    if (state is None) == (u is None):
        raise ValueError("%s: exactly one of state and u must be given" % fn)
    if state is not None:
        if (not isinstance(state, torch.Tensor) or state.dtype != torch.int64
                or state.shape != (2,) or not state.is_contiguous()):
            raise ValueError("%s: state must be a contiguous int64 [2] tensor" % fn)
        if state.device != like.device:
            raise ValueError("%s: state must be on the input's device" % fn)
        return None
    if not isinstance(u, torch.Tensor) or u.dtype != torch.float32:
        raise ValueError("%s: u must be a float32 tensor" % fn)
    if u.dim() != 2 or u.shape[0] != N or u.shape[1] != 2:
        raise ValueError("%s: u must be [%d, 2], got %s" % (fn, N, tuple(u.shape)))
    if u.device != like.device:
        raise ValueError("%s: u must be on the input's device" % fn)
    return u.contiguous()


def _draw_eager(state, N):
    """The uniforms of a launch with `state`, which is advanced."""
    seed, step = (int(v) for v in state.tolist())
    u = philox_uniforms(seed, step, N).to(state.device)
    state[1] = step + 1 if step + 1 < 1 << 63 else step + 1 - (1 << 64)
    return u


def _categorical_eager(logits, u):
    N, A = logits.shape
    m = logits.max(dim=1, keepdim=True).values
    e = torch.exp(logits - m)
    total = torch.zeros(N, dtype=torch.float32, device=logits.device)
    last = torch.zeros(N, dtype=torch.int64, device=logits.device)
    for a in range(A):
        total = total + e[:, a]
        last = torch.where(e[:, a] > 0, a, last)
    target = u[:, 0] * total
    c = torch.zeros_like(total)
    found = torch.zeros(N, dtype=torch.bool, device=logits.device)
    action = last  # rounding at the top: no running sum exceeds target
    for a in range(A):
        c = c + e[:, a]
        hit = (c > target) & ~found
        action = torch.where(hit, a, action)
        found = found | hit
    return action


def sample_categorical(logits, state=None, u=None, out=None):
    """action ~ softmax(logits) for logits float32 [..., A]: int64 [...].

    Exactly one of `state` (int64 [2] on the logits' device, advanced by one)
    and `u` (float32 [N, 2], N the number of rows) drives the draw. `out`, an
    int64 [N] buffer, is written into if given. One launch on the GPU, eager
    torch on the CPU or with MOOLIB_AMD_NO_ACT_KERNEL set.
    """
    fn = "sample_categorical"
    rows = _rows(logits, fn, "logits")
    N = rows.shape[0]
    u = _source(state, u, rows, N, fn)
    k = _kernels() if rows.is_cuda else None
    if k is not None:
        action = k.act_categorical(rows, state, u, out)
    else:
        if u is None:
            u = _draw_eager(state, N)
        action = _categorical_eager(rows, u)
        if out is not None:
            action = out.copy_(action)
    return action.view(logits.shape[:-1])


def _eps_greedy_eager(value, adv, epsilon, u):
    N, A = adv.shape
    s = torch.zeros(N, dtype=torch.float32, device=adv.device)
    for a in range(A):
        s = s + adv[:, a]
    mean = s / torch.tensor(float(A), dtype=torch.float32, device=adv.device)
    q = (value.unsqueeze(1) + adv) - mean.unsqueeze(1)
    best = q[:, 0]
    greedy = torch.zeros(N, dtype=torch.int64, device=adv.device)
    for a in range(1, A):
        better = q[:, a] > best  # strict: the lowest index of the maximum wins
        best = torch.where(better, q[:, a], best)
        greedy = torch.where(better, a, greedy)
    explore = u[:, 0] < epsilon
    scaled = u[:, 1] * torch.tensor(float(A), dtype=torch.float32, device=adv.device)
    random_action = torch.floor(scaled).to(torch.int64).clamp(max=A - 1)
    action = torch.where(explore, random_action, greedy)
    q_taken = q.gather(1, action.unsqueeze(1)).squeeze(1)
    return action, q_taken, best


def epsilon_greedy_dueling(value, advantage, epsilon, state=None, u=None, out=None):
    """Epsilon-greedy actions on the dueling Q-values of `value` float32 [...]
    and `advantage` float32 [..., A]: (action int64, q_taken, q_max), each
    [...].

    `epsilon` is a float32 tensor of one exploration rate per row ([...]), or
    a scalar (a number or a 1-element tensor) that broadcasts. Exactly one of
    `state` and `u` drives the draw, as in sample_categorical. `out`, a
    triple of [N] buffers, is written into if given. One launch on the GPU.
    """
    fn = "epsilon_greedy_dueling"
    adv = _rows(advantage, fn, "advantage")
    N = adv.shape[0]
    if not isinstance(value, torch.Tensor) or value.dtype != torch.float32:
        raise ValueError("%s: value must be a float32 tensor" % fn)
    if value.numel() != N or value.device != adv.device:
        raise ValueError("%s: value must hold one element per row of advantage, on its device" % fn)
    value = value.detach().reshape(N).contiguous()
    if isinstance(epsilon, torch.Tensor):
        if epsilon.dtype != torch.float32:
            raise ValueError("%s: epsilon must be a float32 tensor or a number" % fn)
        if epsilon.device != adv.device:
            raise ValueError("%s: epsilon must be on the input's device" % fn)
        if epsilon.numel() == 1:
            epsilon = epsilon.reshape(1).expand(N)
        elif epsilon.numel() != N:
            raise ValueError("%s: %d epsilons for %d rows" % (fn, epsilon.numel(), N))
        epsilon = epsilon.detach().reshape(N).contiguous()
    else:
        epsilon = torch.full((N,), float(epsilon), dtype=torch.float32, device=adv.device)
    u = _source(state, u, adv, N, fn)
    k = _kernels() if adv.is_cuda else None
    if k is not None:
        o = out if out is not None else (None, None, None)
        res = k.act_eps_greedy(value, adv, epsilon, state, u, o[0], o[1], o[2])
    else:
        if u is None:
            u = _draw_eager(state, N)
        res = _eps_greedy_eager(value, adv, epsilon, u)
        if out is not None:
            res = tuple(o.copy_(r) for o, r in zip(out, res))
    shape = advantage.shape[:-1]
    return tuple(r.view(shape) for r in res)
