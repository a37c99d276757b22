"""Device-side prioritized replay: sum tree, stratified sampling, indexed rows.

docs/KERNEL_TESTS.md ("Replay") has the premises, bounds and recorded figures.

* The tree is a pure function of its leaves: after any sequence of updates it
  must be `torch.equal` to a rebuild from its leaves by fp32 pairwise adds.
  Leaves are one rounding (2^-24) of a double pow away from the float64
  reference, whose own rounding doubles that: 2^-23 |ref|.
* Integer premise: integer priorities at alpha = 1, total <= 512, B a power of
  two <= 64 and u a multiple of 2^-8 make every fp32 quantity of the descent
  exact, so the indices must equal a float64 searchsorted of the CDF.
* The CPU tests pin the plain-torch path; the GPU tests require the kernels to
  be `torch.equal` to it (tree, indices, rows) and within the same 2^-23 of
  float64 (leaves, weights), writing into sentinel-filled outputs.
"""
import functools
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

import moolib_amd
import replay_refs as R
from moolib_amd.ops import replay as ops
from moolib_amd.replay import ReplayBuffer, ReplayClient, SumTreeReplayBuffer
from moolib_amd.utils import nest

gpu = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

REL = 2.0 ** -23
CAPACITIES = [1, 2, 3, 5, 1000]
ALPHA = 0.6
U_EDGES = {"zero": 0.0, "top": 1.0 - 2.0 ** -24}


def _figure(**kw):
    """One machine-readable line per measured figure (shown with pytest -s)."""
    print("KERNEL_EDGES_FIGURE " + json.dumps(kw))


def _worst_ratio(got, ref):
    """max |got - ref| / (2^-23 |ref|), got fp32, ref float64."""
    err = (got.double().cpu() - ref).abs()
    return float((err / (REL * ref.abs())).max())


# ------------------------------------------------------------ tree scenarios


@functools.lru_cache(maxsize=None)
def tree_ops(capacity, integer=False):
    """A fixed list of (slots, priorities or None) updates: fresh items at
    max_priority, random slots with duplicates (more than one kernel round,
    and for capacity 1000 more than one launch), the clamp at 1e-6, a large
    priority, ring wrap-around."""
    g = torch.Generator().manual_seed(17 * capacity + int(integer))

    def prios(n, scale):
        if integer:
            return torch.randint(1, 9, (n,), generator=g).float()
        return torch.rand(n, generator=g) * scale

    out = [(torch.arange(max(1, capacity // 2)), None)]
    K = 3 * capacity + 1
    out.append((torch.randint(0, capacity, (K,), generator=g), prios(K, 10.0)))
    if not integer:
        edge = torch.tensor([0.0, 1e6, 1e-7])[: min(3, capacity)]
        out.append((torch.arange(edge.numel()), edge))
    out.append((torch.arange(capacity - 1, capacity + 2) % capacity, None))
    if capacity == 1000:
        K = ops.KERNEL_MAX_UPDATE + 904  # above the per-launch cap
        out.append((torch.randint(0, capacity, (K,), generator=g), prios(K, 100.0)))
    return tuple(out)


def apply_ops(capacity, op_list, alpha, device):
    tree = ops.sumtree_new(capacity, device)
    max_priority = torch.ones(1, device=device)
    for slots, p in op_list:
        ops.sumtree_update(tree, max_priority, slots.to(device),
                           None if p is None else p.to(device), alpha)
    return tree, max_priority


@functools.lru_cache(maxsize=None)
def cpu_tree(capacity, integer=False):
    alpha = 1.0 if integer else ALPHA
    return apply_ops(capacity, tree_ops(capacity, integer), alpha, "cpu")


def check_tree(tree, max_priority, capacity, integer, tag):
    alpha = 1.0 if integer else ALPHA
    L = R.leaf_count(capacity)
    tree = tree.cpu()
    assert tree.shape == (2 * L,)
    leaves = tree[L:L + capacity]
    assert torch.equal(tree, R.rebuild_tree(leaves.numpy(), L))
    raw, mx = R.final_leaves(capacity, [(s.numpy(), None if p is None else p.numpy())
                                        for s, p in tree_ops(capacity, integer)])
    written = torch.from_numpy(~np.isnan(raw))
    assert bool(written.any()) and not leaves[~written].any()  # never written: 0
    ref = R.leaf_ref64(raw[written.numpy()], alpha)
    ratio = _worst_ratio(leaves[written], ref)
    _figure(test=tag, capacity=capacity, integer=integer, leaf_err_over_bound=ratio)
    assert ratio <= 1.0
    if integer:
        assert torch.equal(leaves[written].double(), ref)
    assert float(max_priority.cpu()) == float(mx)


class TestTreeCPU:
    @pytest.mark.parametrize("integer", [False, True])
    @pytest.mark.parametrize("capacity", CAPACITIES)
    def test_invariant_and_leaves(self, capacity, integer):
        tree, max_priority = cpu_tree(capacity, integer)
        check_tree(tree, max_priority, capacity, integer, "cpu_tree")

    def test_new_tree_is_zero_and_rounds_up(self):
        for capacity, L in [(1, 1), (2, 2), (3, 4), (5, 8), (1000, 1024), (1024, 1024)]:
            tree = ops.sumtree_new(capacity)
            assert tree.shape == (2 * L,) and tree.dtype == torch.float32
            assert not tree.any()

    def test_last_occurrence_wins(self):
        tree = ops.sumtree_new(5)
        mp = torch.ones(1)
        ops.sumtree_update(tree, mp, torch.tensor([2, 2, 0, 2]),
                           torch.tensor([1.0, 2.0, 3.0, 4.0]), 1.0)
        assert tree[8:13].tolist() == [3.0, 0.0, 4.0, 0.0, 0.0]
        assert float(tree[1]) == 7.0 and float(mp) == 4.0
        # across kernel rounds and launches
        K = ops.KERNEL_MAX_UPDATE + 1000
        k = torch.arange(K)
        ops.sumtree_update(tree, mp, k % 3, (k + 1).float(), 1.0)
        last = [float(max(j for j in range(K - 3, K) if j % 3 == slot) + 1) for slot in range(3)]
        assert tree[8:13].tolist() == last + [0.0, 0.0]
        assert float(mp) == float(K)

    def test_max_priority_and_default_entry(self):
        buf = SumTreeReplayBuffer(4, alpha=1.0)
        assert buf.max_priority.shape == (1,) and float(buf.max_priority) == 1.0
        buf.add({"x": torch.zeros(2)})  # enters at 1
        buf.add({"x": torch.zeros(2)}, priority=0.25)  # below the maximum: unchanged
        assert float(buf.max_priority) == 1.0
        buf.update_priorities([0], [7.5])
        assert float(buf.max_priority) == 7.5
        buf.add_batch({"x": torch.zeros(2, 2)})  # two items, at 7.5
        assert buf.priorities.tolist() == [7.5, 0.25, 7.5, 7.5]
        buf.update_priorities(torch.tensor([3]), torch.tensor([2.0]))
        assert float(buf.max_priority) == 7.5 and float(buf.priorities[3]) == 2.0

    def test_rejects_malformed(self):
        tree = ops.sumtree_new(4)
        with pytest.raises(RuntimeError):
            ops.sumtree_sample(tree, 0, torch.zeros(2), 0.4)
        with pytest.raises(ValueError):
            ops.sumtree_sample(tree, 2, torch.zeros(ops.KERNEL_MAX_SAMPLE + 1), 0.4)
        with pytest.raises(ValueError):
            ops.sumtree_sample(torch.zeros(6), 2, torch.zeros(2), 0.4)
        with pytest.raises(ValueError):
            ops.sumtree_update(tree, torch.ones(1), torch.tensor([0, 1]), torch.ones(3), 1.0)
        with pytest.raises(RuntimeError):
            SumTreeReplayBuffer(4).sample(2)
        with pytest.raises(ValueError):
            SumTreeReplayBuffer(2).add_batch({"x": torch.zeros(3, 1)})


# ------------------------------------------------------------------ sampling

# (capacity, size, B): integer priorities in 1..8, so total <= 8 * size <= 512
INT_CASES = [(5, 5, 1), (5, 3, 2), (8, 8, 8), (64, 64, 64), (100, 60, 32), (1000, 17, 64)]


@functools.lru_cache(maxsize=None)
def int_sample_case(capacity, size, B):
    g = torch.Generator().manual_seed(1000 * capacity + 10 * size + B)
    p = torch.randint(1, 9, (size,), generator=g).float()
    u = torch.randint(0, 256, (B,), generator=g).float() / 256.0
    return p, u


def tree_from(capacity, priorities, alpha, device):
    tree = ops.sumtree_new(capacity, device)
    mp = torch.ones(1, device=device)
    ops.sumtree_update(tree, mp, torch.arange(priorities.numel(), device=device),
                       priorities.to(device), alpha)
    return tree


def sample_into_sentinels(tree, size, u, beta):
    """sumtree_sample writing into buffers no valid result can equal."""
    B = u.numel()
    idx = torch.full((B,), -12345, dtype=torch.int64, device=tree.device)
    w = torch.full((B,), float("nan"), device=tree.device)
    got = ops.sumtree_sample(tree, size, u, beta, out=(idx, w))
    assert got[0].data_ptr() == idx.data_ptr() and got[1].data_ptr() == w.data_ptr()
    return idx, w


def check_int_premise(capacity, size, B, device):
    p, u = int_sample_case(capacity, size, B)
    total = float(p.sum())
    # the premise, asserted: everything the descent touches is exact in fp32
    assert total <= 512 and B & (B - 1) == 0 and B <= 64
    assert torch.equal(u * 256, (u * 256).round())
    target64 = (torch.arange(B).double() + u.double()) * (total / B)
    assert torch.equal(target64.float().double(), target64)
    assert torch.equal((target64 * 2 ** 14).round(), target64 * 2 ** 14)  # subtractions too
    tree = tree_from(capacity, p, 1.0, device)
    assert float(tree[1]) == total
    idx, _ = sample_into_sentinels(tree, size, u.to(device), 0.4)
    idx = idx.cpu()
    assert torch.equal(idx, R.searchsorted_ref64(p.numpy(), B, u.numpy()))
    counts = torch.bincount(idx, minlength=size).double()
    assert float((counts - B * p.double() / total).abs().max()) < 2
    return idx


def never_empty_cases():
    """name -> (capacity, size, priorities [size], alpha)."""
    g = torch.Generator().manual_seed(5)
    swamped = torch.full((300,), 1e-6)
    swamped[123] = 1e6
    return {
        "partial": (1000, 300, torch.rand(300, generator=g) * 5, ALPHA),
        "full_nonpow2": (1000, 1000, torch.rand(1000, generator=g) * 5, ALPHA),
        "swamped": (1000, 300, swamped, 1.0),
        "tiny": (5, 3, torch.tensor([1e-6, 2.0, 1e-7]), ALPHA),
        "single": (1, 1, torch.tensor([0.3]), ALPHA),
    }


NEVER_EMPTY = never_empty_cases()
SAMPLE_B = [1, 7, 1024]
U_KINDS = ["zero", "top", "rand"]


def make_u(kind, B):
    if kind == "rand":
        return torch.rand(B, generator=torch.Generator().manual_seed(B))
    return torch.full((B,), U_EDGES[kind], dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def cpu_sample(name, B, kind, beta=0.4):
    capacity, size, p, alpha = NEVER_EMPTY[name]
    tree = tree_from(capacity, p, alpha, "cpu")
    idx, w = sample_into_sentinels(tree, size, make_u(kind, B), beta)
    return tree, idx, w


def check_sample(tree, idx, w, name, B, kind, beta, tag):
    capacity, size, _, _ = NEVER_EMPTY[name]
    L = R.leaf_count(capacity)
    tree, idx, w = tree.cpu(), idx.cpu(), w.cpu()
    assert idx.shape == (B,) and w.shape == (B,)
    assert int(idx.min()) >= 0 and int(idx.max()) < size
    assert bool((tree[L + idx] > 0).all())
    ref = R.weights_ref64(tree, L, idx, size, beta)
    ratio = _worst_ratio(w, ref)
    _figure(test=tag, case=name, B=B, u=kind, weight_err_over_bound=ratio)
    assert ratio <= 1.0
    assert float(w.max()) == 1.0 and float(w.min()) > 0


class TestSampleCPU:
    @pytest.mark.parametrize("capacity,size,B", INT_CASES)
    def test_integer_premise(self, capacity, size, B):
        check_int_premise(capacity, size, B, "cpu")

    @pytest.mark.parametrize("p", [1.0, 3.0])
    @pytest.mark.parametrize("capacity,size", [(5, 5), (5, 3), (64, 64), (1000, 37)])
    def test_equal_priorities_draw_every_slot_once(self, capacity, size, p):
        tree = tree_from(capacity, torch.full((size,), p), 1.0, "cpu")
        for seed in range(3):
            u = torch.rand(size, generator=torch.Generator().manual_seed(seed))
            idx, w = ops.sumtree_sample(tree, size, u, 0.4)
            assert torch.equal(idx, torch.arange(size))
            assert torch.equal(w, torch.ones(size))

    @pytest.mark.parametrize("kind", U_KINDS)
    @pytest.mark.parametrize("B", SAMPLE_B)
    @pytest.mark.parametrize("name", sorted(NEVER_EMPTY))
    def test_never_an_empty_slot_and_weights(self, name, B, kind):
        tree, idx, w = cpu_sample(name, B, kind)
        check_sample(tree, idx, w, name, B, kind, 0.4, "cpu_sample")
        capacity = NEVER_EMPTY[name][0]
        assert torch.equal(idx, R.descent_fp32(tree, R.leaf_count(capacity), B, make_u(kind, B)))

    def test_beta_zero_gives_ones(self):
        tree, idx, w = cpu_sample("partial", 7, "rand", 0.0)
        assert torch.equal(w, torch.ones(7))

    def test_stratified_one_draw_per_segment(self):
        capacity, size, p, alpha = NEVER_EMPTY["partial"]
        tree, idx, _ = cpu_sample("partial", 1024, "rand")
        assert bool((idx[1:] >= idx[:-1]).all())  # targets increase with b
        # high priorities are drawn in proportion: counts within 2 of B p / total
        leaves = tree[1024:1024 + size].double()
        counts = torch.bincount(idx, minlength=size).double()
        assert float((counts - 1024 * leaves / leaves.sum()).abs().max()) < 2


# ---------------------------------------------------------------------- rows

ROWS_CAPACITY = 7


def rows_storage(n_leaves=25):
    """Storage leaves [capacity, *item]: every dtype, inner rows of 1, 3, 4,
    16 and 20 bytes, 0-dim items, T in {1, 3}; 25 leaves, so the descriptor
    table (24 per launch) chunks."""
    g = torch.Generator().manual_seed(3)
    c = ROWS_CAPACITY
    base = [
        torch.randint(0, 256, (c, 3, 3), generator=g).to(torch.uint8),   # T=3, 3 B
        torch.rand(c, 1, 4, generator=g) < 0.5,                          # bool, T=1, 4 B
        torch.randint(-2 ** 40, 2 ** 40, (c,), generator=g),             # int64, 0-dim items
        torch.randn(c, 3, 8, generator=g).to(torch.bfloat16),            # T=3, 16 B
        torch.randn(c, 3, 5, generator=g),                               # fp32, T=3, 20 B
        torch.randn(c, 1, 1, generator=g),                               # fp32, T=1, 4 B
        torch.randint(0, 256, (c, 3), generator=g).to(torch.uint8),      # 1-dim items, 1 B
        torch.randn(c, 3, 2, 2, generator=g),                            # fp32, T=3, 16 B
        torch.randn(c, generator=g),                                     # fp32, 0-dim items
        torch.randn(c, 1, 5, generator=g).to(torch.bfloat16),            # T=1, 10 B
    ]
    leaves = [base[i % len(base)].clone() for i in range(n_leaves)]
    for i, t in enumerate(leaves[len(base):]):
        if t.dtype not in (torch.bool,):
            t += 1  # distinct contents per repeat
    return leaves


ROWS_INDEX = {
    "one_last": [ROWS_CAPACITY - 1],
    "one_first": [0],
    "repeated": [0, 0, ROWS_CAPACITY - 1, 3, 3, 0, ROWS_CAPACITY - 1],
    "many": list(range(ROWS_CAPACITY)) * 43,  # 301 items: more than one block
}
SCATTER_SLOTS = {
    "one": [ROWS_CAPACITY - 1],
    "ends": [ROWS_CAPACITY - 1, 0, 3],
    "all": [4, 2, 6, 0, 5, 1, 3],
}


def sentinel_like(t):
    if t.dtype == torch.bool:
        return torch.ones_like(t)
    if t.dtype.is_floating_point:
        return torch.full_like(t, float("nan"))
    return torch.full_like(t, 0x55)


def gather_expected(leaves, idx, time_major):
    idx = torch.tensor(idx)
    out = [t[idx] for t in leaves]
    if time_major:
        out = [t.transpose(0, 1).contiguous() if t.dim() >= 2 else t for t in out]
    return out


def run_gather(device, name, time_major):
    leaves = [t.to(device) for t in rows_storage()]
    idx = torch.tensor(ROWS_INDEX[name], device=device)
    want = gather_expected(rows_storage(), ROWS_INDEX[name], time_major)
    out = [sentinel_like(w).to(device) for w in want]
    got = ops.gather_rows(leaves, idx, time_major=time_major, out=out)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got, out))
    fresh = ops.gather_rows(leaves, idx, time_major=time_major)
    return got, fresh, want


def scatter_items(name, batch_dim):
    """Items to scatter (finite values, so a NaN-free comparison) + expected storage."""
    g = torch.Generator().manual_seed(11)
    slots = torch.tensor(SCATTER_SLOTS[name])
    K = slots.numel()
    storage = rows_storage()
    items, expected = [], []
    for t in storage:
        if t.dtype == torch.bool:
            it = torch.rand((K,) + t.shape[1:], generator=g) < 0.5
        elif t.dtype.is_floating_point:
            it = torch.randn((K,) + t.shape[1:], generator=g).to(t.dtype)
        else:
            it = torch.randint(0, 200, (K,) + t.shape[1:], generator=g).to(t.dtype)
        e = t.clone()
        e[slots] = it
        expected.append(e)
        if batch_dim == 1 and it.dim() >= 2:
            it = it.transpose(0, 1).contiguous()
        items.append(it)
    return storage, items, slots, expected


def run_scatter(device, name, batch_dim):
    storage, items, slots, expected = scatter_items(name, batch_dim)
    storage = [t.to(device) for t in storage]
    ops.scatter_rows(storage, [t.to(device) for t in items], slots.to(device),
                     batch_dim=batch_dim)
    return storage, expected


class TestRowsCPU:
    @pytest.mark.parametrize("time_major", [False, True])
    @pytest.mark.parametrize("name", sorted(ROWS_INDEX))
    def test_gather(self, name, time_major):
        got, fresh, want = run_gather("cpu", name, time_major)
        for a, b, w in zip(got, fresh, want):
            assert a.shape == w.shape and a.dtype == w.dtype
            assert torch.equal(a, w) and torch.equal(b, w)

    @pytest.mark.parametrize("batch_dim", [0, 1])
    @pytest.mark.parametrize("name", sorted(SCATTER_SLOTS))
    def test_scatter(self, name, batch_dim):
        storage, expected = run_scatter("cpu", name, batch_dim)
        for a, e in zip(storage, expected):
            assert torch.equal(a, e)


# -------------------------------------------------------------------- buffer


def seq_items(K, start, T=3):
    """K sequences [K, ...] whose contents name them: start, start+1, ..."""
    ids = torch.arange(start, start + K)
    return {
        "obs": ids.view(K, 1, 1).expand(K, T, 2).float().contiguous(),
        "act": ids.view(K, 1).expand(K, T).contiguous(),
        "tag": ids.clone(),
        "core": (ids.view(K, 1, 1).expand(K, 1, 4).to(torch.bfloat16).contiguous(),),
    }


def to_time_major(items):
    return nest.map(lambda t: t.transpose(0, 1).contiguous() if t.dim() >= 2 else t, items)


def buffers_equal(a, b):
    assert a.cursor == b.cursor and a.size == b.size
    assert torch.equal(a.tree.cpu(), b.tree.cpu())
    assert torch.equal(a.max_priority.cpu(), b.max_priority.cpu())
    for x, y in zip(nest.flatten(a.storage), nest.flatten(b.storage)):
        assert torch.equal(x.cpu(), y.cpu())


def fill_ring(device, capacity, batch_dim):
    """Three add_batch calls that wrap the ring; written slots only."""
    buf = SumTreeReplayBuffer(capacity, device=device, alpha=1.0, beta=0.4)
    start, slots = 0, []
    for K in [min(3, capacity), min(2, capacity), min(3, capacity)]:
        items = seq_items(K, start)
        if batch_dim == 1:
            items = to_time_major(items)
        items = nest.map(lambda t: t.to(device), items)
        slots.append(buf.add_batch(items, batch_dim=batch_dim))
        start += K
    return buf, start, slots


class TestBufferCPU:
    @pytest.mark.parametrize("capacity", [1, 2, 3, 5, 8])
    def test_ring_keeps_the_newest(self, capacity):
        buf, n, slots = fill_ring("cpu", capacity, 0)
        assert len(buf) == min(n, capacity) and buf.cursor == n % capacity
        assert all(s.dtype == torch.int64 for s in slots)
        L = R.leaf_count(capacity)
        assert torch.equal(buf.tree, R.rebuild_tree(buf.priorities.numpy(), L))
        # equal priorities, B == size: every slot once
        batch, idx, w = buf.sample(len(buf), u=torch.rand(len(buf)))
        assert torch.equal(idx, torch.arange(len(buf)))
        newest = list(range(n - len(buf), n))
        assert sorted(batch["tag"].tolist()) == newest
        for key in ("obs", "act"):
            assert torch.equal(batch[key].reshape(len(buf), -1)[:, 0].long(), batch["tag"])
        assert torch.equal(batch["core"][0][:, 0, 0].long(), batch["tag"])
        # slot of item i is i % capacity
        assert torch.equal(batch["tag"] % capacity, idx)

    def test_batch_dim_1_equals_batch_dim_0(self):
        a, _, sa = fill_ring("cpu", 5, 0)
        b, _, sb = fill_ring("cpu", 5, 1)
        buffers_equal(a, b)
        assert all(torch.equal(x, y) for x, y in zip(sa, sb))

    def test_add_is_add_batch_of_one(self):
        a = SumTreeReplayBuffer(4, alpha=0.7)
        b = SumTreeReplayBuffer(4, alpha=0.7)
        prios = [None, 0.5, 3.0, None, 0.1, None]
        for i, p in enumerate(prios):
            item = nest.map(lambda t: t[0], seq_items(1, i))
            assert a.add(item, p) == i % 4
            slots = b.add_batch(seq_items(1, i), None if p is None else torch.tensor([p]))
            assert slots.tolist() == [i % 4]
        buffers_equal(a, b)

    def test_time_major_sample_and_reproducible(self):
        buf, _, _ = fill_ring("cpu", 8, 0)
        buf.update_priorities(torch.arange(8), torch.arange(1, 9).float())
        u = torch.rand(6, generator=torch.Generator().manual_seed(1))
        bm, idx, w = buf.sample(6, u=u)
        tm, idx2, w2 = buf.sample(6, time_major=True, u=u)
        assert torch.equal(idx, idx2) and torch.equal(w, w2)
        assert tm["obs"].shape == (3, 6, 2) and tm["act"].shape == (3, 6)
        assert tm["tag"].shape == (6,) and tm["core"][0].shape == (1, 6, 4)
        for x, y in zip(nest.flatten(bm), nest.flatten(tm)):
            assert torch.equal(x.transpose(0, 1) if x.dim() >= 2 else x, y)
        g1 = buf.sample(6, generator=torch.Generator().manual_seed(9))[1]
        g2 = buf.sample(6, generator=torch.Generator().manual_seed(9))[1]
        assert torch.equal(g1, g2)

    def test_base_buffer_gains_add_batch_and_time_major(self):
        buf = ReplayBuffer(8, alpha=1.0)
        slots = buf.add_batch(to_time_major(seq_items(3, 0)), batch_dim=1)
        assert slots.tolist() == [0, 1, 2] and len(buf) == 3
        assert buf.storage["tag"][:3].tolist() == [0, 1, 2]
        assert torch.equal(buf.storage["obs"][:3], seq_items(3, 0)["obs"])
        batch, idx, w = buf.sample(4, time_major=True)
        assert batch["obs"].shape == (3, 4, 2) and batch["tag"].shape == (4,)
        assert torch.equal(batch["obs"][0, :, 0].long(), idx)

    def test_served_add_batch_and_time_major_sample(self):
        server = moolib_amd.Rpc()
        server.set_name("sumtree_server")
        addr = server.listen("127.0.0.1:0")[0]
        buf = SumTreeReplayBuffer(16, alpha=1.0).serve(server, "replay")
        client_rpc = moolib_amd.Rpc()
        client_rpc.set_name("sumtree_learner")
        client_rpc.set_timeout(15)
        client_rpc.connect(addr)
        client = ReplayClient(client_rpc, "sumtree_server", "replay")

        slots = client.add_batch(to_time_major(seq_items(5, 0)), None, 1).result()
        assert slots.tolist() == [0, 1, 2, 3, 4]
        slots = client.add_batch(seq_items(2, 5), torch.tensor([2.0, 3.0])).result()
        assert slots.tolist() == [5, 6] and client.info()["size"] == 7
        client.add(nest.map(lambda t: t[0], seq_items(1, 7))).result()
        assert len(buf) == 8 and float(buf.max_priority) == 3.0

        batch, idx, w = client.sample(6, True).result()
        assert batch["obs"].shape == (3, 6, 2) and batch["core"][0].shape == (1, 6, 4)
        assert torch.equal(batch["tag"], idx) and w.shape == (6,)
        batch, idx, w = client.sample_ipc(4, True).result()
        assert batch["act"].shape == (3, 4)
        batch, idx, w = client.sample(4).result()
        assert batch["obs"].shape == (4, 3, 2)
        client.update_priorities(idx, torch.full((4,), 9.0)).result()
        assert float(buf.max_priority) == 9.0


class TestExamplesCPU:
    def _examples(self):
        path = os.path.join(os.path.dirname(__file__), "..", "examples")
        if path not in sys.path:
            sys.path.insert(0, path)

    def test_r2d2_replay_sumtree(self):
        self._examples()
        import r2d2_replay

        m = r2d2_replay.run(device="cpu", capacity=64, unroll=5, batch_size=4, num_envs=4,
                            seconds=2.0, sumtree=True)
        assert m["sumtree"] is True
        assert m["buffer_seqs"] >= 4 and m["buffer_seqs"] % 4 == 0  # num_envs per unroll
        assert m["sampled"] > 0

    def test_r2d2_sumtree(self):
        self._examples()
        import r2d2

        m = r2d2.run(device="cpu", capacity=64, unroll=3, burn_in=1, batch_size=4, num_envs=4,
                     seconds=2.0, sumtree=True)
        assert m["sumtree"] is True and m["buffer_seqs"] >= 4
        assert m["learn_steps"] > 0 and math.isfinite(m["loss"])


# =============================================================== GPU tests


@gpu
@requires_gpu
class TestKernels:
    @pytest.mark.parametrize("integer", [False, True])
    @pytest.mark.parametrize("capacity", CAPACITIES)
    def test_tree_equals_eager(self, capacity, integer):
        alpha = 1.0 if integer else ALPHA
        tree, max_priority = apply_ops(capacity, tree_ops(capacity, integer), alpha, "cuda")
        want_tree, want_max = cpu_tree(capacity, integer)
        check_tree(tree, max_priority, capacity, integer, "kernel_tree")
        assert torch.equal(tree.cpu(), want_tree)
        assert torch.equal(max_priority.cpu(), want_max)
        again, _ = apply_ops(capacity, tree_ops(capacity, integer), alpha, "cuda")
        assert torch.equal(again, tree)

    def test_last_occurrence_wins(self):
        tree = ops.sumtree_new(5, "cuda")
        mp = torch.ones(1, device="cuda")
        K = ops.KERNEL_MAX_UPDATE + 1000
        k = torch.arange(K, device="cuda")
        ops.sumtree_update(tree, mp, k % 3, (k + 1).float(), 1.0)
        last = [float(max(j for j in range(K - 3, K) if j % 3 == slot) + 1) for slot in range(3)]
        assert tree[8:13].tolist() == last + [0.0, 0.0]
        assert float(mp) == float(K)

    @pytest.mark.parametrize("capacity,size,B", INT_CASES)
    def test_integer_premise(self, capacity, size, B):
        idx = check_int_premise(capacity, size, B, "cuda")
        assert torch.equal(idx, check_int_premise(capacity, size, B, "cpu"))

    @pytest.mark.parametrize("kind", U_KINDS)
    @pytest.mark.parametrize("B", SAMPLE_B)
    @pytest.mark.parametrize("name", sorted(NEVER_EMPTY))
    def test_sample_equals_eager(self, name, B, kind):
        capacity, size, p, alpha = NEVER_EMPTY[name]
        want_tree, want_idx, _ = cpu_sample(name, B, kind)
        tree = tree_from(capacity, p, alpha, "cuda")
        assert torch.equal(tree.cpu(), want_tree)
        u = make_u(kind, B).cuda()
        idx, w = sample_into_sentinels(tree, size, u, 0.4)
        assert torch.equal(idx.cpu(), want_idx)
        check_sample(tree, idx, w, name, B, kind, 0.4, "kernel_sample")
        idx2, w2 = sample_into_sentinels(tree, size, u, 0.4)
        assert torch.equal(idx2, idx) and torch.equal(w2, w)

    def test_beta_zero_and_batch_limit(self):
        capacity, size, p, alpha = NEVER_EMPTY["partial"]
        tree = tree_from(capacity, p, alpha, "cuda")
        idx, w = sample_into_sentinels(tree, size, make_u("rand", 7).cuda(), 0.0)
        assert torch.equal(w.cpu(), torch.ones(7))
        B = ops.KERNEL_MAX_SAMPLE
        idx, w = sample_into_sentinels(tree, size, make_u("rand", B).cuda(), 0.4)
        want = ops.sumtree_sample(tree.cpu(), size, make_u("rand", B), 0.4)[0]
        assert torch.equal(idx.cpu(), want)

    @pytest.mark.parametrize("time_major", [False, True])
    @pytest.mark.parametrize("name", sorted(ROWS_INDEX))
    def test_gather_equals_eager(self, name, time_major):
        got, fresh, want = run_gather("cuda", name, time_major)
        for a, b, w in zip(got, fresh, want):
            assert a.shape == w.shape and a.dtype == w.dtype
            assert torch.equal(a.cpu(), w) and torch.equal(b.cpu(), w)

    @pytest.mark.parametrize("batch_dim", [0, 1])
    @pytest.mark.parametrize("name", sorted(SCATTER_SLOTS))
    def test_scatter_equals_eager(self, name, batch_dim):
        storage, expected = run_scatter("cuda", name, batch_dim)
        for a, e in zip(storage, expected):
            assert torch.equal(a.cpu(), e)

    def test_buffer_equals_cpu_buffer(self):
        for batch_dim in (0, 1):
            a, _, _ = fill_ring("cuda", 5, batch_dim)
            b, _, _ = fill_ring("cpu", 5, batch_dim)
            buffers_equal(a, b)
            u = torch.rand(4, generator=torch.Generator().manual_seed(2))
            for tm in (False, True):
                x, xi, xw = a.sample(4, time_major=tm, u=u.cuda())
                y, yi, yw = b.sample(4, time_major=tm, u=u)
                assert torch.equal(xi.cpu(), yi)
                for s, t in zip(nest.flatten(x), nest.flatten(y)):
                    assert torch.equal(s.cpu(), t)

    def test_eager_gpu_path_on_request(self, monkeypatch):
        monkeypatch.setenv("MOOLIB_AMD_NO_REPLAY_KERNEL", "1")
        tree, max_priority = apply_ops(5, tree_ops(5), ALPHA, "cuda")
        assert torch.equal(tree.cpu(), cpu_tree(5)[0])

    def test_no_host_wait(self):
        buf, _, _ = fill_ring("cuda", 8, 1)  # storage allocated, kernels loaded
        items = nest.map(lambda t: t.cuda(), to_time_major(seq_items(3, 100)))
        prios = torch.tensor([1.0, 2.0, 3.0], device="cuda")
        u = torch.rand(4, device="cuda")
        torch.cuda.synchronize()
        mode = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            slots = buf.add_batch(items, prios, batch_dim=1)
            batch, idx, w = buf.sample(4, time_major=True, u=u)
            buf.sample(4)  # default u: torch.rand on the device
            buf.update_priorities(idx, w)
        finally:
            torch.cuda.set_sync_debug_mode(mode)
        assert slots.is_cuda and idx.is_cuda and w.is_cuda
        assert torch.equal(buf.tree.cpu(),
                           R.rebuild_tree(buf.priorities.cpu().numpy(), R.leaf_count(8)))

    def test_feeds_the_learner(self):
        from moolib_amd.r2d2 import R2D2Config, R2D2Learner

        T, B, N, A = 6, 4, 8, 3
        torch.manual_seed(0)
        learner = R2D2Learner(_TinyNet(A), R2D2Config(lr=1e-2, burn_in=1, n_step=2), "cuda")
        g = torch.Generator().manual_seed(4)
        unroll = {
            "state": torch.randn(T, N, 4, generator=g),
            "reward": torch.randn(T, N, generator=g),
            "done": torch.rand(T, N, generator=g) < 0.15,
            "prev_action": torch.randint(0, A, (T, N), generator=g),
            "action": torch.randint(0, A, (T, N), generator=g),
            "core_h": 0.1 * torch.randn(1, N, 8, generator=g),
            "core_c": 0.1 * torch.randn(1, N, 8, generator=g),
        }
        buf = SumTreeReplayBuffer(16, device="cuda", alpha=0.9, beta=0.6)
        buf.add_batch(nest.map(lambda t: t.cuda(), unroll), batch_dim=1)
        items, idx, w = buf.sample(B, time_major=True)
        assert items["state"].shape == (T, B, 4) and items["core_h"].shape == (1, B, 8)
        batch = {k: items[k] for k in ("state", "reward", "done", "prev_action", "action")}
        batch["core_state"] = (items["core_h"], items["core_c"])
        metrics, priorities = learner.learn(batch, w)
        assert priorities.shape == (B,) and bool(torch.isfinite(priorities).all())
        buf.update_priorities(idx, priorities)
        L = R.leaf_count(16)
        assert torch.equal(buf.tree.cpu(), R.rebuild_tree(buf.priorities.cpu().numpy(), L))
        want = R.leaf_ref64(priorities.cpu().numpy(), 0.9)
        # repeated indices: the last occurrence holds the leaf
        last = {int(s): k for k, s in enumerate(idx.tolist())}
        for s, k in last.items():
            got = float(buf.priorities[s])
            assert abs(got - float(want[k])) <= REL * float(want[k])
        assert float(buf.max_priority) == max(1.0, float(priorities.max()))


class _TinyNet(torch.nn.Module):
    """Stand-in with AtariNet's forward contract: [T,B,4] float state, an LSTM
    core reset where done, policy_logits / baseline heads."""

    def __init__(self, num_actions=3):
        super().__init__()
        self.num_actions = num_actions
        self.fc = torch.nn.Linear(4 + 1 + num_actions, 8)
        self.core = torch.nn.LSTM(8, 8)
        self.policy = torch.nn.Linear(8, num_actions)
        self.baseline = torch.nn.Linear(8, 1)

    def initial_state(self, batch_size=1):
        return tuple(torch.zeros(1, batch_size, 8) for _ in range(2))

    def forward(self, inputs, core_state):
        T, B = inputs["reward"].shape
        onehot = torch.nn.functional.one_hot(inputs["prev_action"], self.num_actions).float()
        x = torch.cat([inputs["state"], inputs["reward"].unsqueeze(-1), onehot], dim=-1)
        x = torch.relu(self.fc(x))
        outs = []
        for t in range(T):
            nd = (~inputs["done"][t]).float().view(1, B, 1)
            core_state = tuple(nd * s for s in core_state)
            o, core_state = self.core(x[t:t + 1], core_state)
            outs.append(o)
        y = torch.cat(outs)
        out = {"policy_logits": self.policy(y), "baseline": self.baseline(y).squeeze(-1)}
        return out, core_state
