"""References for the action-head tests, written from the definition in
moolib_amd/ops/act.py and not from the op: Philox4x32-10 on Python integers,
the epsilon-greedy dueling head with every fp32 operation formed in fp64 and
rounded once (for +, -, *, / of fp32 operands that IS the IEEE fp32 result,
fp64 having more than 2*24+2 bits), and the categorical CDF in fp64.
"""
import numpy as np

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF


def philox4x32(counter, key, rounds=10):
    """The four output words of Philox4x32 for a counter and a key of 32-bit
    Python integers."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(rounds):
        p0 = 0xD2511F53 * c0
        p1 = 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0 = (k0 + 0x9E3779B9) & M32
        k1 = (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def counter_and_key(seed, step, row):
    seed &= M64
    step &= M64
    return (row, 0, step & M32, step >> 32), (seed & M32, seed >> 32)


def words(seed, step, row):
    """Raw Philox words of one row of a launch."""
    return philox4x32(*counter_and_key(seed, step, row))


def uniforms(seed, step, rows):
    """(u0, u1) of the given rows: float32 [len(rows), 2]."""
    out = np.empty((len(rows), 2), dtype=np.float32)
    for i, row in enumerate(rows):
        x = words(seed, step, int(row))
        out[i, 0] = (x[0] >> 8) / 2.0 ** 24
        out[i, 1] = (x[1] >> 8) / 2.0 ** 24
    return out


def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def _f64(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def eps_greedy_ref(value, advantage, epsilon, u):
    """(action int64 [N], q_taken float32 [N], q_max float32 [N]) of numpy
    float32 inputs value [N], advantage [N, A], epsilon [N], u [N, 2]."""
    value, advantage, epsilon, u = (np.asarray(t, dtype=np.float32)
                                    for t in (value, advantage, epsilon, u))
    N, A = advantage.shape
    s = np.zeros(N, dtype=np.float32)
    for a in range(A):
        s = _f32(_f64(s) + _f64(advantage[:, a]))
    mean = _f32(_f64(s) / float(A))
    q = np.empty((N, A), dtype=np.float32)
    for a in range(A):
        q[:, a] = _f32(_f64(_f32(_f64(value) + _f64(advantage[:, a]))) - _f64(mean))
    greedy = np.zeros(N, dtype=np.int64)
    for n in range(N):
        for a in range(1, A):
            if q[n, a] > q[n, greedy[n]]:
                greedy[n] = a
    explore = u[:, 0] < epsilon
    scaled = _f32(_f64(u[:, 1]) * float(A))
    random_action = np.minimum(A - 1, np.floor(_f64(scaled)).astype(np.int64))
    action = np.where(explore, random_action, greedy)
    rows = np.arange(N)
    return action, q[rows, action], q[rows, greedy]


def categorical_cdf(logits):
    """The fp64 CDF of softmax(logits) for float32 logits [N, A]: (C [N, A]
    running sums of exp(l - max), total [N]). -inf logits have mass 0."""
    l = _f64(logits)
    e = np.exp(l - l.max(axis=1, keepdims=True))
    C = np.cumsum(e, axis=1)
    return C, C[:, -1].copy()


def categorical_ref(logits, u0):
    """(action [N], margin [N], nearest [N]) of the fp64 reference: the first
    a with C_a > u0 * total; margin = min_k |u0 total - C_k| / total and
    `nearest` the k that attains it."""
    C, total = categorical_cdf(logits)
    t = _f64(u0) * total
    above = C > t[:, None]
    action = np.where(above.any(axis=1), above.argmax(axis=1), C.shape[1] - 1)
    dist = np.abs(t[:, None] - C) / total[:, None]
    return action.astype(np.int64), dist.min(axis=1), dist.argmin(axis=1)


def masked_categorical_ref(logits, u0):
    """Exact action for logits in {0, -inf}: every e_a is 0 or 1, so fp32
    running sums are exact integers and only `u0 * total` rounds (once)."""
    logits = np.asarray(logits, dtype=np.float32)
    N, A = logits.shape
    out = np.empty(N, dtype=np.int64)
    for n in range(N):
        e = [1 if logits[n, a] == 0 else 0 for a in range(A)]
        total = sum(e)
        target = np.float32(np.float64(u0[n]) * total)
        c, pick = 0, max(a for a in range(A) if e[a])
        for a in range(A):
            c += e[a]
            if c > target:
                pick = a
                break
        out[n] = pick
    return out
