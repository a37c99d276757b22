#!/usr/bin/env python
"""Micro-timing of the actor's initial priorities: the fused kernel path of
ops.r2d2.actor_priorities (one HIP launch) against the eager torch path
(MOOLIB_AMD_NO_R2D2_KERNEL) on the same GPU, in the same process, on the same
seeded inputs, the variants alternating.

At [80, 64] and [40, 16] (T, K), n-step 5, uncaptured and as the replay of a
one-call torch.cuda.graph.

After a warm-up each call is bracketed by device events; a window of calls
ended by a device synchronise gives the wall time per call, which is what a
launch-bound chain costs the host. Reported: the median and the p10-p90 spread
of the per-call device times over all rounds, the wall time per call of every
round, the device launches of one call of each path (torch.profiler) and the
largest difference between the two paths' outputs. Nothing is asserted.

Run on an MI355X:  python tools/actor_priority_micro.py
                   (writes profiles/actor_priority_micro.txt)
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
from moolib_amd.ops import r2d2

WARMUP, ITERS, ROUNDS = 20, 100, 3
SHAPES = [(80, 64), (40, 16)]  # (T, K)
KWARGS = dict(n_step=5, discount=0.997, eps=1e-3, eta=0.9, burn_in=0)


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


def launches(fn):
    """Device launches (kernels and copies) of one call."""
    try:
        from torch.profiler import ProfilerActivity, profile

        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events()
                 if e.device_type == torch.autograd.DeviceType.CUDA]
        return str(len(names)) if names else "n/a"
    except Exception as e:  # noqa: BLE001 — the count is a courtesy, the timing is the point
        return "n/a (%s)" % type(e).__name__


def captured(fn):
    """`fn` as the replay of a one-call graph."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = fn()
    return lambda keep=keep: g.replay()  # the outputs live as long as the graph


def compare(label, fns, emit):
    for fn in fns.values():
        timed(fn, WARMUP)
    times = {k: [] for k in fns}
    walls = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            per_call, wall = timed(fn, ITERS)
            times[k] += per_call
            walls[k].append(wall)
    emit(label)
    for k in fns:
        q = statistics.quantiles(times[k], n=10)
        emit("  %-16s device %8.1f us (p10-p90 %.1f-%.1f)   wall us per call, per round: %s"
             % (k, statistics.median(times[k]), q[0], q[-1],
                " ".join("%.1f" % w for w in walls[k])))
    med = {k: statistics.median(v) for k, v in times.items()}
    wall = {k: statistics.median(v) for k, v in walls.items()}
    emit("  eager/fused: device %.2fx, wall %.2fx;  eager_graph/fused_graph: device %.2fx, wall %.2fx"
         % (med["eager"] / med["fused"], wall["eager"] / wall["fused"],
            med["eager_graph"] / med["fused_graph"], wall["eager_graph"] / wall["fused_graph"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "actor_priority_micro.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("actor_priority_micro: needs a GPU; a CPU timing says nothing about it")
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    emit("device: %s" % torch.cuda.get_device_name(0))
    emit("us per call, %d warm-up + %d x %d timed calls each, the variants alternating"
         % (WARMUP, ROUNDS, ITERS))
    for T, K in SHAPES:
        g = torch.Generator().manual_seed(T)
        q = torch.randn(2, T, K, generator=g)
        q_taken, q_max = q.min(dim=0).values.cuda(), q.max(dim=0).values.cuda()
        reward = torch.randn(T, K, generator=g).cuda()
        done = (torch.rand(T, K, generator=g) < 0.1).cuda()

        def fused():
            os.environ.pop("MOOLIB_AMD_NO_R2D2_KERNEL", None)
            return r2d2.actor_priorities(q_taken, q_max, reward, done, **KWARGS)

        def eager():
            os.environ["MOOLIB_AMD_NO_R2D2_KERNEL"] = "1"
            return r2d2.actor_priorities(q_taken, q_max, reward, done, **KWARGS)

        a, b = fused(), eager()
        fns = {
            "eager": eager,
            "fused": fused,
            "eager_graph": captured(eager),
            "fused_graph": captured(fused),
        }
        emit("launches per call: eager %s, fused %s (uncaptured);  max|priority diff| %.2g, "
             "max|td diff| %.2g"
             % (launches(eager), launches(fused),
                float((a.priorities - b.priorities).abs().max()),
                float((a.td_errors - b.td_errors).abs().max())))
        compare("actor_priorities [%d, %d] n_step %d" % (T, K, KWARGS["n_step"]), fns, emit)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
