#!/usr/bin/env python
"""Micro-timing of the trunk's FC layer (32 x 11 x 11 features -> 256), from the
channels_last bf16 tensor the last conv section hands over:

  eager   F.relu (the trunk's trailing relu), reshape(M, -1) (the layout copy to
          NCHW order), F.linear, relu: what AtariNet runs with
          fused_trunk_fc=False. An fp32 weight runs under autocast, which casts
          it to bf16 on every call; a bf16 weight (shadow weights) runs as is.
  fused   ops.fc.trunk_fc(relu_in=True) (hip/fc.hip.inc).

Shapes: P = 121, M = 128 and 256 (actor), 672 (IMPALA learner, 21 x 32), 5120
(R2D2 learner, 80 x 64). Each is timed forward-only under no_grad and
forward+backward (feat.backward(G); gradients to x, weight and bias), as eager
launches and as one replay of a captured graph. After a warm-up every call is
bracketed by device events and a round ends in a device synchronise; the two
routes alternate over the rounds. Reported: median and p10-p90 of the per-call
device time, and the largest difference between the two routes' outputs on the
same seeded inputs. --split-k S... adds forward rows of the fused route with
that split forced. Nothing is asserted.

Run on an MI355X:  python tools/trunk_fc_micro.py   (writes profiles/trunk_fc_micro.txt)
"""
import argparse
import contextlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from moolib_amd import _kernels  # noqa: F401  (no kernel, no measurement)
from moolib_amd.ops.fc import trunk_fc, trunk_fc_eager

WARMUP, ITERS, ROUNDS = 5, 10, 3
SHAPES = [("actor", 128), ("actor", 256), ("IMPALA learner", 672), ("R2D2 learner", 5120)]
HW = (11, 11)
BF16 = torch.bfloat16


def timed(fn, iters):
    pairs = []
    for _ in range(iters):
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        pairs.append((s, e))
    torch.cuda.synchronize()
    return [s.elapsed_time(e) * 1000.0 for s, e in pairs]


def captured(fn):
    """fn as one graph replay (warmed up on a side stream first)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph.replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trunk_fc_micro.txt"))
    ap.add_argument("--split-k", type=int, nargs="*", default=[])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("trunk_fc_micro: needs a GPU; a CPU timing says nothing about it")

    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    emit("device: %s" % torch.cuda.get_device_name(0))
    emit("%d warm-up + %d x %d timed calls each, the routes alternating; device us, median (p10-p90)"
         % (WARMUP, ROUNDS, ITERS))
    for name, M in SHAPES:
        for wdtype in (torch.float32, BF16):
            torch.manual_seed(0)
            fc = torch.nn.Linear(32 * HW[0] * HW[1], 256).cuda().to(wdtype)
            x = torch.randn(M, 32, *HW, device="cuda").to(BF16)
            x = x.contiguous(memory_format=torch.channels_last).requires_grad_()
            G = torch.randn(M, 256, device="cuda").to(BF16)
            amp = ((lambda: torch.autocast("cuda", dtype=BF16)) if wdtype == torch.float32
                   else contextlib.nullcontext)

            def route(op, **kw):
                def fwd():
                    with torch.no_grad(), amp():
                        return op(x, fc.weight, fc.bias, True, **kw)

                def train():
                    x.grad = None
                    fc.zero_grad(set_to_none=True)
                    with amp():
                        feat = op(x, fc.weight, fc.bias, True)
                    feat.backward(G)

                return {"fwd": fwd, "fwd+bwd": train}

            fns = {}
            for rname, op in (("eager", trunk_fc_eager), ("fused", trunk_fc)):
                for mode, fn in route(op).items():
                    fns[rname, mode, "launches"] = fn
            for s in args.split_k:
                fns["fused S=%d" % s, "fwd", "launches"] = route(trunk_fc, split_k=s)["fwd"]
            diff = (fns["eager", "fwd", "launches"]().float()
                    - fns["fused", "fwd", "launches"]().float()).abs().max().item()
            for (rname, mode, _), fn in list(fns.items()):
                fns[rname, mode, "graph"] = captured(fn)
            for fn in fns.values():
                timed(fn, WARMUP)
            times = {k: [] for k in fns}
            for _ in range(ROUNDS):
                for k, fn in fns.items():
                    times[k] += timed(fn, ITERS)
            emit("%s: M=%d P=%d weight %s; max|feat_fused - feat_eager| = %.4f"
                 % (name, M, HW[0] * HW[1], str(wdtype).replace("torch.", ""), diff))
            for how in ("launches", "graph"):
                for mode in ("fwd", "fwd+bwd"):
                    cells = []
                    for rname in sorted({k[0] for k in fns if k[1:] == (mode, how)}):
                        t = times[rname, mode, how]
                        q = statistics.quantiles(t, n=10)
                        cells.append("%s %8.1f (%.1f-%.1f)" % (rname, statistics.median(t), q[0], q[-1]))
                    ratio = (statistics.median(times["eager", mode, how])
                             / statistics.median(times["fused", mode, how]))
                    emit("  %-8s %-8s %s   eager/fused %.2fx" % (how, mode, "   ".join(cells), ratio))

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
