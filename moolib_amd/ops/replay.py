"""Device-side prioritized replay: a float32 sum tree with stratified
sampling (Schaul et al. 2016), and indexed gather / scatter of whole nests.

Sum tree. `L` is the capacity rounded up to a power of two; `tree` is
float32[2L], `tree[1]` the root, `tree[L + slot]` the leaves, `tree[0]`
unused, never-written leaves 0, and every internal node exactly

    tree[n] = fl32(tree[2n] + tree[2n+1])

so the whole tree is a pure function of its leaves.

    leaf_k   = (float) pow((double) max(p_k, 1e-6f), (double) alpha)
    total    = tree[1],  seg = total / (float) B          (fp32 division)
    target_b = ((float) b + u_b) * seg                    (stratified, one per segment)
    descent  : go right iff tree[right] > 0 and (target >= tree[left] or tree[left] == 0),
               subtracting tree[left] from target on the way right
    w_b      = pow((double) size * p_b / total, -beta) / max_b (...)   in double, rounded once

The descent rule never returns an empty slot while total > 0, even when fp32
rounding pushes a target to `total` or a 1e-6 leaf sits next to a 1e6 one.

On an MI355X each op is one launch of a HIP kernel of moolib_amd._kernels
(replay_tree_update, replay_tree_sample, replay_rows; one launch per
KERNEL_MAX_LEAVES leaves for the rows), and none waits for the device. The
plain-torch path below is the CPU implementation and the reference of the
kernel tests: it performs the same operations in the same order.
"""
import os

import torch

# Most slots one replay_tree_update launch takes (_kernels.REPLAY_MAX_UPDATE is
# the same number); sumtree_update chunks longer lists in order, so the last
# occurrence of a slot still wins.
KERNEL_MAX_UPDATE = 4096
# Largest batch sumtree_sample draws (_kernels.REPLAY_MAX_SAMPLE); larger ones
# are rejected, not rerouted.
KERNEL_MAX_SAMPLE = 4096

_MIN_PRIORITY = 1e-6


def _kernels():
    """The kernel module for a GPU call, or None if the eager path was asked
    for. A build without the kernels is an error on the GPU, not a quiet
    detour through eager launches."""
    if os.environ.get("MOOLIB_AMD_NO_REPLAY_KERNEL"):
        return None
    try:
        from moolib_amd import _kernels as k
    except ImportError as e:
        raise ImportError(
            "replay ops on a GPU tensor need moolib_amd._kernels (python setup.py build_ext "
            "--inplace); set MOOLIB_AMD_NO_REPLAY_KERNEL=1 to run the eager path instead"
        ) from e
    return k


def _leaf_count(tree):
    if tree.dim() != 1 or tree.dtype != torch.float32 or tree.numel() < 2:
        raise ValueError("sum tree must be a float32 vector of 2L elements")
    L = tree.numel() // 2
    if 2 * L != tree.numel() or L & (L - 1):
        raise ValueError("sum tree must have 2L elements with L a power of two")
    return L


def sumtree_new(capacity, device="cpu"):
    """An all-zero tree for `capacity` slots: float32[2L]."""
    capacity = int(capacity)
    if capacity < 1:
        raise ValueError("sumtree_new: capacity must be >= 1, got %d" % capacity)
    L = 1 << (capacity - 1).bit_length()
    return torch.zeros(2 * L, dtype=torch.float32, device=device)


def _update_eager(tree, max_priority, slots, priorities, alpha, L):
    K = slots.numel()
    if priorities is None:
        p = max_priority.expand(K)
    else:
        p = priorities
    leaf = p.clamp_min(_MIN_PRIORITY).double().pow(alpha).float()
    # Last occurrence wins: give every occurrence of a slot the value of its
    # last one (stable sort keeps the order of equal slots), so the indexed
    # store below does not depend on which duplicate lands.
    order = torch.argsort(slots, stable=True)
    s = slots[order]
    last = torch.searchsorted(s, s, right=True) - 1
    winner = torch.empty_like(leaf)
    winner[order] = leaf[order[last]]
    tree[L + slots] = winner
    node = L + slots
    for _ in range(L.bit_length() - 1):
        node = node >> 1
        tree[node] = tree[2 * node] + tree[2 * node + 1]
    if priorities is not None:
        max_priority.copy_(torch.maximum(max_priority, p.max().reshape(1)))


def sumtree_update(tree, max_priority, slots, priorities, alpha):
    """Set the leaves of `slots` (int64 [K], values in [0, capacity)) to
    max(p, 1e-6)^alpha and recompute their ancestors, in place.

    `priorities` is float32 [K], or None for "enter at the current
    `max_priority`" (a 1-element float32 tensor on the tree's device, raised
    to max(old, max_k p_k) on raw priorities). Where a slot occurs more than
    once the last occurrence wins.
    """
    L = _leaf_count(tree)
    alpha = float(alpha)
    slots = slots.to(torch.int64).reshape(-1).contiguous()
    if priorities is not None:
        priorities = priorities.detach().float().reshape(-1).contiguous()
        if priorities.numel() != slots.numel():
            raise ValueError(
                "sumtree_update: %d priorities for %d slots" % (priorities.numel(), slots.numel())
            )
    if max_priority.numel() != 1 or max_priority.dtype != torch.float32:
        raise ValueError("sumtree_update: max_priority must be a 1-element float32 tensor")
    k = _kernels() if tree.is_cuda else None
    for lo in range(0, slots.numel(), KERNEL_MAX_UPDATE):
        s = slots[lo:lo + KERNEL_MAX_UPDATE]
        p = None if priorities is None else priorities[lo:lo + KERNEL_MAX_UPDATE]
        if k is not None:
            k.replay_tree_update(tree, max_priority, s, p, alpha, L)
        else:
            _update_eager(tree, max_priority, s, p, alpha, L)


def _sample_eager(tree, L, size, u, beta):
    B = u.numel()
    total = tree[1]
    seg = total / torch.tensor(float(B), dtype=torch.float32, device=tree.device)
    target = (torch.arange(B, dtype=torch.float32, device=tree.device) + u) * seg
    node = torch.ones(B, dtype=torch.int64, device=tree.device)
    for _ in range(L.bit_length() - 1):
        left = 2 * node
        tl = tree[left]
        tr = tree[left + 1]
        right = (tr > 0) & ((target >= tl) | (tl == 0))
        target = torch.where(right, target - tl, target)
        node = torch.where(right, left + 1, left)
    idx = node - L
    w = (float(size) * tree[node].double() / total.double()).pow(-float(beta))
    w = (w / w.max()).float()
    return idx, w


def sumtree_sample(tree, size, u, beta, out=None):
    """Stratified sample of B = len(u) slots among the first `size`.

    `u` is float32 [B] in [0, 1): draw b lands in the b-th of B equal-mass
    segments of the priority CDF. Returns (idx int64 [B], weights float32
    [B]), the weights (size * P(i))^-beta divided by their batch maximum.
    `size` is a host integer. `out=(idx, weights)` writes into existing
    buffers.
    """
    L = _leaf_count(tree)
    size = int(size)
    if size < 1:
        raise RuntimeError("sumtree_sample: the tree is empty (size == 0)")
    if size > L:
        raise ValueError("sumtree_sample: size %d exceeds the tree's %d leaves" % (size, L))
    if u.dim() != 1 or u.numel() < 1:
        raise ValueError("sumtree_sample: u must be a non-empty vector")
    if u.numel() > KERNEL_MAX_SAMPLE:
        raise ValueError(
            "sumtree_sample: batch of %d exceeds the limit of %d" % (u.numel(), KERNEL_MAX_SAMPLE)
        )
    if u.device != tree.device:
        raise ValueError("sumtree_sample: u must be on the tree's device")
    u = u.float().contiguous()
    k = _kernels() if tree.is_cuda else None
    if k is not None:
        idx_out, w_out = out if out is not None else (None, None)
        idx, w = k.replay_tree_sample(tree, L, size, u, float(beta), idx_out, w_out)
        return idx, w
    idx, w = _sample_eager(tree, L, size, u, beta)
    if out is not None:
        out[0].copy_(idx)
        out[1].copy_(w)
        return out[0], out[1]
    return idx, w


def _time_major(t):
    """Leaves with a time axis: storage [capacity, T, ...], items [T, ...]."""
    return t.dim() >= 2


def gather_rows(leaves, idx, time_major=False, out=None):
    """out[b] = leaf[idx[b]] for every storage leaf [capacity, ...] of the
    list `leaves`; with `time_major`, out[t, b] = leaf[idx[b], t] (leaves of
    0-dim items stay [B]). One launch for all leaves on the GPU. `out` is an
    optional list of buffers to fill."""
    leaves = list(leaves)
    idx = idx.to(torch.int64).reshape(-1).contiguous()
    B = idx.numel()
    if out is None:
        out = []
        for t in leaves:
            shape = (B,) + tuple(t.shape[1:])
            if time_major and _time_major(t):
                shape = (t.shape[1], B) + tuple(t.shape[2:])
            out.append(torch.empty(shape, dtype=t.dtype, device=t.device))
    out = list(out)
    if not leaves:
        return out
    k = _kernels() if leaves[0].is_cuda else None
    if k is not None:
        k.replay_rows(leaves, out, idx, 1 if time_major else 0)
        return out
    for t, o in zip(leaves, out):
        rows = t[idx]
        if time_major and _time_major(t):
            rows = rows.transpose(0, 1)
        o.copy_(rows)
    return out


def scatter_rows(storage_leaves, item_leaves, slots, batch_dim=0):
    """storage[slots[k]] = items[k] for every leaf pair, in place; with
    `batch_dim=1` the items are time-major, storage[slots[k], t] =
    items[t, k]. `slots` must hold distinct values in [0, capacity). One
    launch for all leaves on the GPU."""
    if batch_dim not in (0, 1):
        raise ValueError("scatter_rows: batch_dim must be 0 or 1, got %r" % (batch_dim,))
    storage_leaves = list(storage_leaves)
    item_leaves = list(item_leaves)
    if len(storage_leaves) != len(item_leaves):
        raise ValueError("scatter_rows: %d storage leaves, %d item leaves"
                         % (len(storage_leaves), len(item_leaves)))
    slots = slots.to(torch.int64).reshape(-1).contiguous()
    if not storage_leaves:
        return
    k = _kernels() if storage_leaves[0].is_cuda else None
    if k is not None:
        k.replay_rows(storage_leaves, [t.contiguous() for t in item_leaves], slots,
                      3 if batch_dim == 1 else 2)
        return
    for dst, src in zip(storage_leaves, item_leaves):
        if batch_dim == 1 and _time_major(dst):
            src = src.transpose(0, 1)
        dst[slots] = src
