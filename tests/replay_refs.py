"""References for the sum-tree replay tests, written from the definitions in
docs/KERNEL_TESTS.md ("Replay"), not from moolib_amd/ops/replay.py.

numpy scalars do the fp32 arithmetic (every np.float32 operation is one IEEE
rounding), Python floats the float64 arithmetic.
"""
import numpy as np
import torch

F32 = np.float32
MIN_PRIORITY = F32(1e-6)


def leaf_count(capacity):
    L = 1
    while L < capacity:
        L *= 2
    return L


def rebuild_tree(leaves, L):
    """float32[2L] tree from its leaves by fp32 pairwise adds; tree[0] = 0."""
    leaves = np.asarray(leaves, dtype=F32)
    tree = np.zeros(2 * L, dtype=F32)
    tree[L:L + len(leaves)] = leaves
    for n in range(L - 1, 0, -1):
        tree[n] = F32(tree[2 * n] + tree[2 * n + 1])
    return torch.from_numpy(tree)


def leaf_ref64(priorities, alpha):
    """max(p, 1e-6f)^alpha in float64 (not rounded to fp32), p given as fp32."""
    p = np.maximum(np.asarray(priorities, dtype=F32), MIN_PRIORITY).astype(np.float64)
    return torch.from_numpy(np.power(p, float(alpha)))


def final_leaves(capacity, ops, initial_max=1.0):
    """Replay a list of (slots, priorities or None) updates one element at a
    time. Returns (raw priority per slot as fp32, or NaN if never written;
    max_priority)."""
    raw = np.full(capacity, np.nan, dtype=F32)
    mx = F32(initial_max)
    for slots, prios in ops:
        slots = np.asarray(slots)
        if prios is None:
            for s in slots:
                raw[s] = mx
        else:
            prios = np.asarray(prios, dtype=F32)
            for s, p in zip(slots, prios):
                raw[s] = p  # later occurrences overwrite: last wins
            mx = max(mx, prios.max())
    return raw, mx


def descent_fp32(tree, L, B, u):
    """The stratified descent, one draw at a time, in fp32 scalars."""
    tree = tree.numpy()
    u = np.asarray(u, dtype=F32)
    total = tree[1]
    seg = F32(total / F32(B))
    out = []
    for b in range(B):
        target = F32(F32(F32(b) + F32(u[b])) * seg)
        node = 1
        while node < L:
            left, right = 2 * node, 2 * node + 1
            if tree[right] > 0 and (target >= tree[left] or tree[left] == 0):
                target = F32(target - tree[left])
                node = right
            else:
                node = left
        out.append(node - L)
    return torch.tensor(out, dtype=torch.int64)


def searchsorted_ref64(priorities, B, u):
    """Stratified inverse-CDF sample in float64: the first slot whose
    cumulative priority exceeds target_b = (b + u_b) total / B."""
    p = np.asarray(priorities, dtype=np.float64)
    cdf = np.cumsum(p)
    target = (np.arange(B, dtype=np.float64) + np.asarray(u, dtype=np.float64)) * (cdf[-1] / B)
    return torch.from_numpy(np.searchsorted(cdf, target, side="right").astype(np.int64))


def weights_ref64(tree, L, idx, size, beta):
    """(size p / total)^-beta / max in float64, p and total read from the fp32 tree."""
    t = tree.double()
    w = (float(size) * t[L + idx] / t[1]).pow(-float(beta))
    return w / w.max()
