"""Distributed prioritized replay, resident in GPU HBM.

BASELINE.json config 5: "R2D2-style distributed prioritized replay resident
in 288 GB HBM (stresses tensor RPC)". A ReplayBuffer peer preallocates its
ring storage on the learner GPU — 288 GB HBM3E holds ~40M Atari frames
(uint8 84x84x4) without ever touching host memory — and serves add/sample
over the moolib RPC plane (tensors ride the wire out-of-band, staged
through pinned host memory on the GPU boundary).

Proportional prioritization (Schaul et al. 2016): P(i) ~ p_i^alpha, with
importance weights w_i = (N * P(i))^-beta / max w.
"""
import torch

from moolib_amd import ipc
from moolib_amd.ops import replay as replay_ops
from moolib_amd.utils import nest


def _leaf_batch_dim(t, batch_dim):
    """Leaves of 0-dim items ([K] stacked) have no time axis to sit behind."""
    return batch_dim if t.dim() > batch_dim else 0


class ReplayBuffer:
    """Ring buffer of fixed-shape sequence nests with proportional priorities.

    Can be used locally or served over RPC with `serve()`.
    """

    def __init__(self, capacity, device="cpu", alpha=0.6, beta=0.4):
        self.capacity = int(capacity)
        self.device = torch.device(device)
        self.alpha = alpha
        self.beta = beta
        self.storage = None  # nest of [capacity, ...] tensors
        self.priorities = torch.zeros(self.capacity, dtype=torch.float32, device=self.device)
        self.cursor = 0
        self.size = 0
        self.max_priority = 1.0

    def _ensure_storage(self, item):
        if self.storage is not None:
            return
        def alloc(t):
            return torch.empty(
                (self.capacity,) + tuple(t.shape), dtype=t.dtype, device=self.device
            )
        self.storage = nest.map(alloc, item)

    def add(self, item, priority=None):
        """Insert one sequence nest; returns its slot index."""
        item = nest.map(lambda t: torch.as_tensor(t), item)
        self._ensure_storage(item)
        idx = self.cursor
        for dst, src in zip(nest.flatten(self.storage), nest.flatten(item)):
            dst[idx].copy_(src.to(self.device, non_blocking=True))
        p = float(priority) if priority is not None else self.max_priority
        self.priorities[idx] = max(p, 1e-6) ** self.alpha
        self.max_priority = max(self.max_priority, p)
        self.cursor = (self.cursor + 1) % self.capacity
        self.size = min(self.size + 1, self.capacity)
        return idx

    def add_batch(self, items, priorities=None, batch_dim=0):
        """Insert the K sequences stacked along `batch_dim` of every leaf, one
        `add` each; returns their slots as a tensor."""
        leaves = [torch.as_tensor(t) for t in nest.flatten(items)]
        K = leaves[0].shape[_leaf_batch_dim(leaves[0], batch_dim)]
        if priorities is not None:
            priorities = torch.as_tensor(priorities).reshape(-1).tolist()
        slots = []
        for k in range(K):
            item = nest.map(
                lambda t: torch.as_tensor(t).select(_leaf_batch_dim(t, batch_dim), k), items
            )
            slots.append(self.add(item, None if priorities is None else priorities[k]))
        return torch.tensor(slots, dtype=torch.int64)

    def sample(self, batch_size, time_major=False):
        """Returns (batch nest [B, ...], indices [B], is_weights [B]); with
        `time_major` the leaves that have a time axis come back [T, B, ...]."""
        if self.size == 0:
            raise RuntimeError("replay buffer is empty")
        probs = self.priorities[: self.size]
        idx = torch.multinomial(probs, batch_size, replacement=True)
        batch = nest.map(lambda t: t[idx], self.storage)
        if time_major:
            batch = nest.map(
                lambda t: t.transpose(0, 1).contiguous() if t.dim() >= 2 else t, batch
            )
        psum = probs.sum()
        p = probs[idx] / psum
        w = (self.size * p).pow(-self.beta)
        w = w / w.max().clamp_min(1e-12)
        return batch, idx, w

    def update_priorities(self, indices, priorities):
        indices = torch.as_tensor(indices, device=self.device, dtype=torch.int64)
        priorities = torch.as_tensor(priorities, device=self.device, dtype=torch.float32)
        self.priorities[indices] = priorities.clamp_min(1e-6) ** self.alpha
        self.max_priority = max(self.max_priority, float(priorities.max()))

    def __len__(self):
        return self.size

    # ----------------------------------------------------------- serving

    def serve(self, rpc, name="replay"):
        """Expose this buffer on an Rpc peer."""

        def add(item, priority=None):
            return self.add(item, priority)

        def add_batch(items, priorities=None, batch_dim=0):
            return self.add_batch(items, priorities, batch_dim).cpu()

        def sample(batch_size, time_major=False):
            batch, idx, w = self.sample(batch_size, time_major=time_major)
            # Tensors cross the wire on the CPU; receivers move them where
            # they want. Same-node consumers use `.sample_ipc` instead.
            return (
                nest.map(lambda t: t.cpu(), batch),
                idx.cpu(),
                w.cpu(),
            )

        def sample_ipc(batch_size, time_major=False):
            # Zero-copy for same-node consumers: device tensors ship as
            # hipIpc handles (moolib_amd.ipc); idx/weights are tiny, CPU.
            batch, idx, w = self.sample(batch_size, time_major=time_major)
            if self.device.type == "cuda":
                batch = nest.map(ipc.share, batch)
            else:
                batch = nest.map(lambda t: t.cpu(), batch)
            return (batch, idx.cpu(), w.cpu())

        def update_priorities(indices, priorities):
            self.update_priorities(indices, priorities)

        def info():
            return {"size": self.size, "capacity": self.capacity}

        rpc.define(name + ".add", add)
        rpc.define(name + ".add_batch", add_batch)
        rpc.define(name + ".sample", sample)
        rpc.define(name + ".sample_ipc", sample_ipc)
        rpc.define(name + ".update_priorities", update_priorities)
        rpc.define(name + ".info", info)
        return self


class SumTreeReplayBuffer(ReplayBuffer):
    """ReplayBuffer whose priorities live in a device-side sum tree
    (moolib_amd.ops.replay): stratified sampling, and `add_batch`, `sample`
    and `update_priorities` are a fixed, small number of kernel launches each,
    independent of the capacity and of the number of nest leaves, none of
    which waits for the device.

    `max_priority` is a 1-element tensor on the buffer's device; `cursor` and
    `size` stay host integers. `priorities` is the view of the tree's leaves.

    A priority update for a slot that was overwritten since it was sampled is
    applied to the new occupant, as in ReplayBuffer; generation tags are out
    of scope.
    """

    def __init__(self, capacity, device="cpu", alpha=0.6, beta=0.4):
        super().__init__(capacity, device=device, alpha=alpha, beta=beta)
        self.tree = replay_ops.sumtree_new(self.capacity, self.device)
        L = self.tree.numel() // 2
        self.priorities = self.tree[L:L + self.capacity]
        self.max_priority = torch.ones(1, dtype=torch.float32, device=self.device)

    def _to_device(self, t, dtype=None):
        t = torch.as_tensor(t)
        return t.to(device=self.device, dtype=dtype, non_blocking=True)

    def add_batch(self, items, priorities=None, batch_dim=0):
        """Insert K <= capacity sequences at cursor .. cursor+K-1 (modulo the
        capacity): one scatter and one tree update. Every leaf of `items`
        stacks the K sequences along `batch_dim`; `batch_dim=1` takes an
        actor's [T, K, ...] unroll as it is. `priorities` is [K] or None
        (enter at the highest priority seen). Returns the slots, a device
        tensor."""
        if batch_dim not in (0, 1):
            raise ValueError("add_batch: batch_dim must be 0 or 1, got %r" % (batch_dim,))
        leaves = [self._to_device(t) for t in nest.flatten(items)]
        if not leaves:
            raise ValueError("add_batch: empty nest")
        K = leaves[0].shape[_leaf_batch_dim(leaves[0], batch_dim)]
        if not 1 <= K <= self.capacity:
            raise ValueError(
                "add_batch: %d sequences do not fit a capacity of %d" % (K, self.capacity)
            )
        if self.storage is None:
            template = iter([t.select(_leaf_batch_dim(t, batch_dim), 0) for t in leaves])
            self._ensure_storage(nest.map(lambda _: next(template), items))
        storage = list(nest.flatten(self.storage))
        if len(storage) != len(leaves):
            raise ValueError("add_batch: %d leaves, storage has %d" % (len(leaves), len(storage)))
        for dst, src in zip(storage, leaves):
            want = list(dst.shape[1:])
            want.insert(_leaf_batch_dim(src, batch_dim), K)
            if list(src.shape) != want or src.dtype != dst.dtype:
                raise ValueError(
                    "add_batch: leaf of shape %s %s does not match storage %s %s"
                    % (tuple(src.shape), src.dtype, tuple(dst.shape), dst.dtype)
                )
        if priorities is not None:
            priorities = self._to_device(priorities, torch.float32).reshape(-1)
            if priorities.numel() != K:
                raise ValueError("add_batch: %d priorities for %d sequences"
                                 % (priorities.numel(), K))
        slots = torch.arange(self.cursor, self.cursor + K, device=self.device)
        if self.cursor + K > self.capacity:
            slots = slots % self.capacity
        replay_ops.scatter_rows(storage, leaves, slots, batch_dim=batch_dim)
        replay_ops.sumtree_update(self.tree, self.max_priority, slots, priorities, self.alpha)
        self.cursor = (self.cursor + K) % self.capacity
        self.size = min(self.size + K, self.capacity)
        return slots

    def add(self, item, priority=None):
        """Insert one sequence nest (`add_batch` of one); returns its slot."""
        idx = self.cursor
        items = nest.map(lambda t: torch.as_tensor(t).unsqueeze(0), item)
        if priority is not None:
            priority = torch.as_tensor(priority, dtype=torch.float32).reshape(1)
        self.add_batch(items, priority)
        return idx

    def sample(self, batch_size, time_major=False, u=None, generator=None):
        """Stratified sample: returns (batch nest, indices [B], is_weights
        [B]), the batch [B, ...] or, with `time_major`, [T, B, ...] for the
        leaves that have a time axis. `u` (float32 [B] in [0, 1), default
        torch.rand on the buffer's device) places draw b inside the b-th
        equal-mass segment of the priority CDF, so a sample is reproducible
        from `u`."""
        if self.size == 0:
            raise RuntimeError("replay buffer is empty")
        batch_size = int(batch_size)
        if u is None:
            u = torch.rand(batch_size, device=self.device, generator=generator)
        else:
            u = self._to_device(u, torch.float32).reshape(-1)
            if u.numel() != batch_size:
                raise ValueError("sample: u has %d elements for a batch of %d"
                                 % (u.numel(), batch_size))
        idx, w = replay_ops.sumtree_sample(self.tree, self.size, u, self.beta)
        out = iter(replay_ops.gather_rows(nest.flatten(self.storage), idx, time_major))
        return nest.map(lambda _: next(out), self.storage), idx, w

    def update_priorities(self, indices, priorities):
        """Device tensors are taken as they are; nothing is read back."""
        indices = self._to_device(indices, torch.int64).reshape(-1)
        priorities = self._to_device(priorities, torch.float32).reshape(-1)
        replay_ops.sumtree_update(self.tree, self.max_priority, indices, priorities, self.alpha)


class ReplayClient:
    """Client for a remote ReplayBuffer served on peer `server_name`."""

    def __init__(self, rpc, server_name, name="replay"):
        self.rpc = rpc
        self.server = server_name
        self.name = name

    def add(self, item, priority=None):
        return self.rpc.async_(self.server, self.name + ".add", item, priority)

    def add_batch(self, items, priorities=None, batch_dim=0):
        return self.rpc.async_(
            self.server, self.name + ".add_batch", items, priorities, batch_dim
        )

    def sample(self, batch_size, time_major=False):
        return self.rpc.async_(self.server, self.name + ".sample", batch_size, time_major)

    def sample_ipc(self, batch_size, time_major=False):
        """Same-node zero-copy sample: device tensors arrive as hipIpc
        aliases of the server's HBM (do not use across nodes)."""
        return self.rpc.async_(
            self.server, self.name + ".sample_ipc", batch_size, time_major
        )

    def update_priorities(self, indices, priorities):
        return self.rpc.async_(
            self.server, self.name + ".update_priorities", indices, priorities
        )

    def info(self):
        return self.rpc.sync(self.server, self.name + ".info")
