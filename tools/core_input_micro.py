#!/usr/bin/env python
"""Micro-timing of the LSTM input projection, in bf16 under autocast over fp32
parameters (the learner's setting):

  eager   ops.lstm.core_input_eager on the GPU: one_hot, clamp, cat, the bias
          add, the autocast weight cast and F.linear with K = 257 + A, which is
          what AtariNet runs with fused_core_input=False;
  fused   ops.lstm.core_input_projection (hip/lstm_input.hip.inc).

Shapes: M=256 H=256 (IMPALA actor), M=640 H=256 (IMPALA learner), M=5120 H=512
(R2D2 learner), A=18. Each is timed forward-only under no_grad and
forward+backward (loss = (Xg * G).sum(), gradients to feat, weight_ih and both
biases). After a warm-up every call is bracketed by device events and a round
ends in a device synchronise; the two routes alternate over the rounds.
Reported: median and p10-p90 of the per-call device time, and the largest
difference between the two routes' outputs on the same seeded inputs. Nothing
is asserted.

Run on an MI355X:  python tools/core_input_micro.py   (writes profiles/core_input_micro.txt)
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from moolib_amd import _kernels  # noqa: F401  (no kernel, no measurement)
from moolib_amd.ops.lstm import core_input_eager, core_input_projection

WARMUP, ITERS, ROUNDS = 5, 10, 3
SHAPES = [("IMPALA actor", 256, 256), ("IMPALA learner", 640, 256), ("R2D2 learner", 5120, 512)]
A = 18


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "core_input_micro.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("core_input_micro: needs a GPU; a CPU timing says nothing about it")

    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    emit("device: %s" % torch.cuda.get_device_name(0))
    emit("%d warm-up + %d x %d timed calls each, the routes alternating; device us, median (p10-p90)"
         % (WARMUP, ROUNDS, ITERS))
    for name, M, H in SHAPES:
        torch.manual_seed(0)
        core = torch.nn.LSTM(257 + A, H).cuda()
        params = (core.weight_ih_l0, core.bias_ih_l0, core.bias_hh_l0)
        feat = torch.randn(M, 256, device="cuda").relu().to(torch.bfloat16).requires_grad_()
        reward = 2 * torch.randn(M, device="cuda")
        action = torch.randint(0, A, (M,), device="cuda")
        G = torch.randn(M, 4 * H, device="cuda").to(torch.bfloat16)

        def route(op):
            def fwd():
                with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                    return op(feat, reward, action, *params)

            def train():
                feat.grad = None
                core.zero_grad(set_to_none=True)
                with torch.autocast("cuda", dtype=torch.bfloat16):
                    Xg = op(feat, reward, action, *params)
                Xg.backward(G)

            return {"fwd": fwd, "fwd+bwd": train}

        fns = {}
        for rname, op in (("eager", core_input_eager), ("fused", core_input_projection)):
            for mode, fn in route(op).items():
                fns[rname, mode] = fn
        diff = (fns["eager", "fwd"]().float() - fns["fused", "fwd"]().float()).abs().max().item()
        for fn in fns.values():
            timed(fn, WARMUP)
        times = {k: [] for k in fns}
        for _ in range(ROUNDS):
            for k, fn in fns.items():
                times[k] += timed(fn, ITERS)
        emit("%s: M=%d H=%d A=%d; max|Xg_fused - Xg_eager| = %.4f" % (name, M, H, A, diff))
        for mode in ("fwd", "fwd+bwd"):
            cells = []
            for rname in ("eager", "fused"):
                q = statistics.quantiles(times[rname, mode], n=10)
                cells.append("%s %8.1f (%.1f-%.1f)"
                             % (rname, statistics.median(times[rname, mode]), q[0], q[-1]))
            ratio = statistics.median(times["eager", mode]) / statistics.median(times["fused", mode])
            emit("  %-8s %s   eager/fused %.2fx" % (mode, "   ".join(cells), ratio))

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
