#!/usr/bin/env python
"""Micro-timing of the 3x3 conv weight gradient at the IMPALA learner's shapes
(N = 672 = (unroll 20 + 1) x batch 32), three candidates in one process:

  miopen  aten.convolution_backward, weight gradient only, as _Conv3x3Fn calls
          it: with the cast of the fp32 master weight to bf16 in front and the
          cast of the result back to fp32 behind.
  slab    _kernels.wgrad3x3_nhwc plus the reorder to [K, C, 3, 3] (slice, view,
          permute, materialised by one contiguous() copy);
          MOOLIB_AMD_WGRAD_KERNEL=1. For the first conv also channel_sum_fp32.
  splitk  _kernels.wgrad3x3_splitk (hip/wgrad3x3_splitk.hip.inc): dW in
          nn.Conv2d's order, for the first conv with db from the same pass;
          MOOLIB_AMD_WGRAD_KERNEL=2.

The first conv (4 -> 16 on the C = 8 zero-padded activation, with db) has no
miopen row: its default route is `slab`. After a warm-up every call is
bracketed by device events and a round ends in a device synchronise; the
candidates alternate over the rounds. Reported: median and p10-p90 of the
per-call device time and the largest difference between the candidates'
gradients on the same seeded inputs. Nothing is asserted.

Run on an MI355X:  python tools/wgrad_micro.py   (writes profiles/wgrad_micro.txt)
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from moolib_amd import _kernels

WARMUP, ITERS, ROUNDS = 10, 20, 5
N = 672
# (C staged, C of the weight, K, H, W)
SHAPES = [(8, 4, 16, 84, 84), (16, 16, 16, 42, 42), (16, 16, 32, 42, 42), (32, 32, 32, 21, 21),
          (32, 32, 32, 11, 11)]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wgrad_micro.txt"))
    ap.add_argument("--n", type=int, default=N)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("wgrad_micro: needs a GPU; a CPU timing says nothing about it")

    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    emit("device: %s" % torch.cuda.get_device_name(0))
    emit("N=%d; %d warm-up + %d x %d timed calls each, the candidates alternating; "
         "device us, median (p10-p90)" % (args.n, WARMUP, ROUNDS, ITERS))
    for C, cw, K, H, W in SHAPES:
        torch.manual_seed(0)
        x = torch.randn(args.n, C, H, W, device="cuda").to(BF16)
        x = x.contiguous(memory_format=torch.channels_last)
        if cw < C:
            x[:, cw:] = 0
        dy = torch.randn(args.n, K, H, W, device="cuda").to(BF16)
        dy = dy.contiguous(memory_format=torch.channels_last)
        w = torch.randn(K, cw, 3, 3, device="cuda")  # fp32 master weight
        first = cw < C

        def miopen():
            dw = torch.ops.aten.convolution_backward(
                dy, x, w.to(BF16), None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1,
                [False, True, False])[1]
            return dw.to(w.dtype), None

        def slab():
            g = _kernels.wgrad3x3_nhwc(x, dy)[: 9 * C]
            dw = g.view(3, 3, C, K)[:, :, :cw].permute(3, 2, 0, 1).contiguous()
            return dw, (_kernels.channel_sum_fp32(dy) if first else None)

        def splitk():
            dw, db = _kernels.wgrad3x3_splitk(x, dy, cw, first)
            return dw, (db if first else None)

        fns = {"slab": slab, "splitk": splitk}
        if not first:
            fns = {"miopen": miopen, **fns}
        outs = {k: fn() for k, fn in fns.items()}
        ref = outs["splitk"]
        diffs = ["max|dW_%s - dW_splitk| = %.4f" % (k, (o[0] - ref[0]).abs().max().item())
                 for k, o in outs.items() if k != "splitk"]
        if first:
            diffs.append("max|db_slab - db_splitk| = %.4f"
                         % (outs["slab"][1] - ref[1]).abs().max().item())
        for fn in fns.values():
            timed(fn, WARMUP)
        times = {k: [] for k in fns}
        for _ in range(ROUNDS):
            for k, fn in fns.items():
                times[k] += timed(fn, ITERS)
        emit("%d->%d at %dx%d%s (slab rows R=%d, max|dW| = %.1f): %s"
             % (cw, K, H, W, " with db" if first else "",
                _kernels.wgrad3x3_splitk_rows(C, K, W), ref[0].abs().max().item(),
                "; ".join(diffs)))
        med = {k: statistics.median(t) for k, t in times.items()}
        for k, t in times.items():
            q = statistics.quantiles(t, n=10)
            emit("  %-7s %8.1f (%.1f-%.1f)   splitk/%s %.2fx"
                 % (k, med[k], q[0], q[-1], k, med["splitk"] / med[k]))

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
