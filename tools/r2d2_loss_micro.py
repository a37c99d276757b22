#!/usr/bin/env python
"""Micro-timing of the R2D2 loss, forward + backward: the fused kernel path
against the eager torch path (MOOLIB_AMD_NO_R2D2_KERNEL) on the same GPU, in
the same process, on the same inputs, the two alternating.

Each call is bracketed by device events; the figure is the median over the
timed calls after a warm-up (first launches load code objects). The loss is
launch-latency work: what is measured is mostly the number of launches.

Run on an MI355X:  python tools/r2d2_loss_micro.py
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from moolib_amd import _kernels  # noqa: F401  (no kernel, no measurement)
from moolib_amd.ops import r2d2

SHAPES = [(80, 64, 18, 5), (40, 16, 18, 5)]  # (T, B, A, n)
WARMUP, ITERS, ROUNDS = 30, 200, 3


def make_inputs(T, B, A, seed=0):
    g = torch.Generator().manual_seed(seed)
    dev = lambda t: t.cuda()
    return dict(
        q=dev(torch.randn(T, B, A, generator=g)).requires_grad_(True),
        q_target=dev(torch.randn(T, B, A, generator=g)),
        actions=dev(torch.randint(0, A, (T, B), generator=g)),
        rewards=dev(torch.randn(T, B, generator=g)),
        discounts=dev((torch.rand(T, B, generator=g) > 0.1).float() * 0.997),
        mask=dev((torch.rand(T, B, generator=g) > 0.2).float()),
        is_weights=dev(torch.rand(B, generator=g) + 0.1),
    )


def step(inp, n, fused):
    if fused:
        os.environ.pop("MOOLIB_AMD_NO_R2D2_KERNEL", None)
    else:
        os.environ["MOOLIB_AMD_NO_R2D2_KERNEL"] = "1"
    inp["q"].grad = None
    out = r2d2.r2d2_loss(inp["q"], inp["q_target"], inp["actions"], inp["rewards"],
                         inp["discounts"], inp["mask"], inp["is_weights"], n_step=n)
    out.loss.backward()
    return out


def timed(inp, n, fused, iters):
    """Per-call device time in us (one event pair per call) and the wall time
    per call of the whole window, ended by a device synchronise."""
    pairs = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        s.record()
        step(inp, n, fused)
        e.record()
        pairs.append((s, e))
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e6 / iters
    return [s.elapsed_time(e) * 1000.0 for s, e in pairs], wall


def main():
    if not torch.cuda.is_available():
        sys.exit("r2d2_loss_micro: needs a GPU; a CPU timing says nothing about it")
    print("device: %s" % torch.cuda.get_device_name(0))
    print("median us per call (forward + backward), %d warm-up + %d x %d timed calls each, "
          "paths alternating" % (WARMUP, ROUNDS, ITERS))
    ok = True
    for T, B, A, n in SHAPES:
        inp = make_inputs(T, B, A)
        a, b = step(inp, n, True), step(inp, n, False)
        diff = float((a.td_errors - b.td_errors).abs().max())
        for fused in (True, False):
            timed(inp, n, fused, WARMUP)
        times, walls = {True: [], False: []}, {True: [], False: []}
        for _ in range(ROUNDS):
            for fused in (True, False):
                per_call, wall = timed(inp, n, fused, ITERS)
                times[fused] += per_call
                walls[fused].append(wall)
        k, e = statistics.median(times[True]), statistics.median(times[False])
        spread = lambda v: (statistics.quantiles(v, n=10)[0], statistics.quantiles(v, n=10)[-1])
        print("T=%d B=%d A=%d n=%d  kernel %8.1f us (p10-p90 %.1f-%.1f)  eager %8.1f us "
              "(p10-p90 %.1f-%.1f)  eager/kernel %.2fx  max|td diff| %.2g"
              % ((T, B, A, n, k) + spread(times[True]) + (e,) + spread(times[False])
                 + (e / k, diff)))
        print("    wall us per call, per round:  kernel %s  eager %s"
              % (" ".join("%.1f" % w for w in walls[True]),
                 " ".join("%.1f" % w for w in walls[False])))
        ok = ok and k <= e
    if not ok:
        sys.exit("r2d2_loss_micro: the kernel path is SLOWER than the eager path")


if __name__ == "__main__":
    main()
