#!/usr/bin/env python
"""Micro-timing of the actor's action head: the fused kernels of ops.act (one
HIP launch each) against the eager torch ops they replace, on the same GPU, in
the same process, on the same seeded inputs, the variants alternating.

  categorical   ops.act.sample_categorical(logits, state)      vs
                torch.multinomial(softmax(logits), 1)           (AtariNet.forward)
  eps_greedy    ops.act.epsilon_greedy_dueling(v, adv, eps, state)   vs
                dueling_q + argmax + rand + < + randint_like + where (R2D2Learner.act)

at [256, 18] and [672, 18], uncaptured and inside a torch.cuda.graph (where the
eager ops draw from the default generator, which the capture registers).

After a warm-up each call is bracketed by device events; a window of calls
ended by a device synchronise gives the wall time per call, which is what a
launch-bound chain costs the host. Reported: the median and the p10-p90 spread
of the per-call device times over all rounds, the wall time per call of every
round, and the device launches of one call of each path (torch.profiler).
Nothing is asserted.

Run on an MI355X:  python tools/act_head_micro.py   (writes profiles/act_head_micro.txt)
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch
import torch.nn.functional as F

from moolib_amd import _kernels  # noqa: F401  (no kernel, no measurement)
from moolib_amd.ops import act as act_ops
from moolib_amd.ops.r2d2 import dueling_q

WARMUP, ITERS, ROUNDS = 20, 100, 3
SHAPES = [(256, 18), (672, 18)]
EPSILON = 0.05


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "act_head_micro.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("act_head_micro: needs a GPU; a CPU timing says nothing about it")
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    emit("device: %s" % torch.cuda.get_device_name(0))
    emit("us per call, %d warm-up + %d x %d timed calls each, the variants alternating"
         % (WARMUP, ROUNDS, ITERS))
    for N, A in SHAPES:
        g = torch.Generator().manual_seed(N)
        logits = torch.randn(N, A, generator=g).cuda()
        value = torch.randn(N, generator=g).cuda()
        eps = torch.full((N,), EPSILON, device="cuda")

        def make_categorical():
            state = act_ops.new_state(1, "cuda")

            def eager():
                return torch.multinomial(F.softmax(logits, dim=-1), num_samples=1)

            def fused():
                return act_ops.sample_categorical(logits, state=state)

            return eager, fused

        def make_eps_greedy():
            state = act_ops.new_state(1, "cuda")

            def eager():
                q = dueling_q(value, logits)
                action = q.argmax(dim=-1)
                explore = torch.rand(action.shape, device=action.device) < EPSILON
                random_action = torch.randint_like(action, A)
                return torch.where(explore, random_action, action)

            def fused():
                return act_ops.epsilon_greedy_dueling(value, logits, eps, state=state)

            return eager, fused

        for name, make in (("categorical", make_categorical), ("eps_greedy", make_eps_greedy)):
            eager, fused = make()
            eager_g, fused_g = make()
            fns = {
                "eager": eager,
                "fused": fused,
                "eager_graph": captured(eager_g),
                "fused_graph": captured(fused_g),
            }
            emit("launches per call: eager %s, fused %s (%s, uncaptured)"
                 % (launches(eager), launches(fused), name))
            compare("%s [%d, %d]" % (name, N, A), fns, emit)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
