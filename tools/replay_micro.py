#!/usr/bin/env python
"""Micro-timing of the prioritized replay: SumTreeReplayBuffer (device-side
sum tree, one launch per step) against ReplayBuffer (eager torch) on the same
GPU, in the same process, on the same seeded contents, the two alternating.

Timed: `add` of 32 sequences of examples/r2d2.py's item nest at unroll 40
(ReplayBuffer: 32 add calls; SumTreeReplayBuffer: one add_batch(batch_dim=1) of
the actor's [T, 32, ...] unroll), `sample` and `update_priorities` at B in
{16, 64} and capacity 2048, and a priorities-only case at capacity 2^20 with a
one-float payload. `sample` returns what each example consumes: batch-major
from ReplayBuffer (the example transposes views), time-major from the sum tree.

After a warm-up each call is bracketed by device events; a window of calls
ended by a device synchronise gives the wall time per call (ReplayBuffer's
update_priorities waits for the device itself). Reported: the median and the
p10-p90 spread of the per-call device times over all rounds, and the wall time
per call of every round. No speed-up is asserted.

Run on an MI355X:  python tools/replay_micro.py   (writes profiles/replay_micro.txt)
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from moolib_amd import _kernels  # noqa: F401  (no kernel, no measurement)
from moolib_amd.replay import ReplayBuffer, SumTreeReplayBuffer

UNROLL, NUM_ENVS, HIDDEN = 40, 32, 256
WARMUP, ITERS, ROUNDS = 10, 50, 3
ALPHA, BETA = 0.9, 0.6


def unroll_nest(seed, T=UNROLL, K=NUM_ENVS):
    """What examples/r2d2.py stores per unroll: [T, K, ...] plus [1, K, H] state."""
    g = torch.Generator().manual_seed(seed)
    nest = {
        "state": torch.randint(0, 256, (T, K, 4, 84, 84), generator=g).to(torch.uint8),
        "reward": torch.randn(T, K, generator=g),
        "done": torch.rand(T, K, generator=g) < 0.02,
        "prev_action": torch.randint(0, 18, (T, K), generator=g),
        "action": torch.randint(0, 18, (T, K), generator=g),
        "core_h": torch.randn(1, K, HIDDEN, generator=g),
        "core_c": torch.randn(1, K, HIDDEN, generator=g),
    }
    return {k: v.cuda() for k, v in nest.items()}


def float_nest(seed, K):
    g = torch.Generator().manual_seed(seed)
    return {"x": torch.randn(K, generator=g).cuda()}


def per_sequence(nest, batch_dim):
    """The K single-sequence items ReplayBuffer.add takes, sliced beforehand."""
    K = next(iter(nest.values())).shape[batch_dim]
    return [{k: v.select(batch_dim, i).contiguous() for k, v in nest.items()} for i in range(K)]


def timed(fn, iters):
    pairs = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        pairs.append((s, e))
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e6 / iters
    return [s.elapsed_time(e) * 1000.0 for s, e in pairs], wall


def compare(label, tree_fn, base_fn, emit):
    fns = {"sumtree": tree_fn, "eager": base_fn}
    for fn in fns.values():
        timed(fn, WARMUP)
    times = {k: [] for k in fns}
    walls = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            per_call, wall = timed(fn, ITERS)
            times[k] += per_call
            walls[k].append(wall)
    med = {k: statistics.median(v) for k, v in times.items()}
    spread = lambda v: (statistics.quantiles(v, n=10)[0], statistics.quantiles(v, n=10)[-1])
    emit("%-34s sumtree %8.1f us (p10-p90 %.1f-%.1f)  eager %8.1f us (p10-p90 %.1f-%.1f)  "
         "eager/sumtree %.2fx"
         % ((label, med["sumtree"]) + spread(times["sumtree"]) + (med["eager"],)
            + spread(times["eager"]) + (med["eager"] / med["sumtree"],)))
    emit("    wall us per call, per round:  sumtree %s  eager %s"
         % (" ".join("%.1f" % w for w in walls["sumtree"]),
            " ".join("%.1f" % w for w in walls["eager"])))


def fill(tree_buf, base_buf, nest_fn, batch_dim, K):
    """The same seeded sequences and priorities into both buffers."""
    g = torch.Generator().manual_seed(99)
    for step in range(tree_buf.capacity // K):
        nest = nest_fn(step)
        prios = (torch.rand(K, generator=g) * 4 + 0.01).cuda()
        tree_buf.add_batch(nest, prios, batch_dim=batch_dim)
        base_buf.add_batch(nest, prios, batch_dim=batch_dim)
    assert len(tree_buf) == len(base_buf) == tree_buf.capacity
    same = torch.allclose(tree_buf.priorities, base_buf.priorities, rtol=1e-6, atol=0)
    assert same, "the two buffers hold different priorities"


def sample_and_update(tag, tree_buf, base_buf, emit):
    for B in (16, 64):
        compare("%s sample B=%d" % (tag, B),
                lambda: tree_buf.sample(B, time_major=True),
                lambda: base_buf.sample(B), emit)
        g = torch.Generator().manual_seed(B)
        idx = torch.randint(0, tree_buf.capacity, (B,), generator=g).cuda()
        prios = (torch.rand(B, generator=g) * 4 + 0.01).cuda()
        compare("%s update_priorities B=%d" % (tag, B),
                lambda: tree_buf.update_priorities(idx, prios),
                lambda: base_buf.update_priorities(idx, prios), emit)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_micro.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("replay_micro: needs a GPU; a CPU timing says nothing about it")
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    emit("device: %s" % torch.cuda.get_device_name(0))
    emit("median us per call (device events), %d warm-up + %d x %d timed calls each, the two "
         "buffers alternating" % (WARMUP, ROUNDS, ITERS))

    # ---- the example's item nest, capacity 2048
    cap = 2048
    tree_buf = SumTreeReplayBuffer(cap, device="cuda", alpha=ALPHA, beta=BETA)
    base_buf = ReplayBuffer(cap, device="cuda", alpha=ALPHA, beta=BETA)
    one = unroll_nest(0)
    fill(tree_buf, base_buf, lambda step: one, 1, NUM_ENVS)
    items = per_sequence(one, 1)

    def base_add():
        for item in items:
            base_buf.add(item)

    compare("r2d2 nest add 32 x unroll %d" % UNROLL,
            lambda: tree_buf.add_batch(one, batch_dim=1), base_add, emit)
    sample_and_update("r2d2 nest cap=%d" % cap, tree_buf, base_buf, emit)
    del tree_buf, base_buf, one, items
    torch.cuda.empty_cache()

    # ---- priorities only: one float per item, capacity 2^20
    cap = 1 << 20
    tree_buf = SumTreeReplayBuffer(cap, device="cuda", alpha=ALPHA, beta=BETA)
    base_buf = ReplayBuffer(cap, device="cuda", alpha=ALPHA, beta=BETA)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(cap, generator=g).cuda()
    prios = (torch.rand(cap, generator=g) * 4 + 0.01).cuda()
    tree_buf.add_batch({"x": x}, prios)
    # ReplayBuffer.add is one call per item: set the same contents directly
    base_buf.add({"x": x[0]})
    base_buf.storage["x"].copy_(x)
    base_buf.priorities.copy_(prios.clamp_min(1e-6).double().pow(ALPHA).float())
    base_buf.size, base_buf.cursor = cap, 0
    base_buf.max_priority = float(prios.max())
    assert torch.allclose(tree_buf.priorities, base_buf.priorities, rtol=1e-6, atol=0)
    small = float_nest(1, NUM_ENVS)
    small_items = per_sequence(small, 0)

    def base_add_small():
        for item in small_items:
            base_buf.add(item)

    compare("one float add 32, cap=2^20", lambda: tree_buf.add_batch(small), base_add_small, emit)
    sample_and_update("one float cap=2^20", tree_buf, base_buf, emit)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
