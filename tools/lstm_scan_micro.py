#!/usr/bin/env python
"""Micro-timing of the masked LSTM core at a hidden size the wide scan kernels
serve (default: R2D2's 512 units, unroll 80, batch 64), in bf16:

  loop        the per-step Python loop over nn.LSTM that AtariNet runs when no
              scan kernel serves the size (input projection included);
  fused       F.linear for x @ W_ih^T + b over all T, then ops.lstm.fused_lstm_scan;
  scan        fused_lstm_scan alone on a precomputed X.

Each is timed forward+backward (loss = H.sum() + hT.sum() + cT.sum()) and
forward-only under no_grad. After a warm-up every call is bracketed by device
events and a round ends in a device synchronise; the variants alternate over
the rounds. Reported: median and p10-p90 of the per-call device time, and the
wall time per call of each round. Nothing is asserted.

Run on an MI355X:  python tools/lstm_scan_micro.py   (writes profiles/lstm_scan_micro.txt)
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
from moolib_amd.ops.lstm import fused_lstm_scan

WARMUP, ITERS, ROUNDS = 3, 10, 3


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--T", type=int, default=80)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstm_scan_micro.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lstm_scan_micro: needs a GPU; a CPU timing says nothing about it")
    T, B, Hd, I = args.T, args.B, args.hidden, 256 + 18 + 1

    torch.manual_seed(0)
    core = torch.nn.LSTM(I, Hd).cuda().to(torch.bfloat16)
    x = torch.randn(T, B, I, device="cuda").to(torch.bfloat16)
    done = torch.rand(T, B, device="cuda") < 0.02
    nd_f = (~done).float()
    nd_b = (~done).to(torch.bfloat16)
    h0 = (0.3 * torch.randn(B, Hd, device="cuda")).to(torch.bfloat16)
    c0 = 0.3 * torch.randn(B, Hd, device="cuda")
    X_pre = F.linear(x, core.weight_ih_l0, core.bias_ih_l0 + core.bias_hh_l0).detach()

    def loop():
        state = (h0.unsqueeze(0), c0.unsqueeze(0).to(torch.bfloat16))
        outs = []
        for t in range(T):
            m = nd_b[t].view(1, -1, 1)
            state = tuple(m * s for s in state)
            out_t, state = core(x[t : t + 1], state)
            outs.append(out_t)
        return torch.cat(outs), state[0][0], state[1][0]

    def fused():
        X = F.linear(x, core.weight_ih_l0, core.bias_ih_l0 + core.bias_hh_l0)
        return fused_lstm_scan(X, nd_f, h0, c0, core.weight_hh_l0)

    def scan():
        return fused_lstm_scan(X_pre, nd_f, h0, c0, core.weight_hh_l0)

    def train(f):
        def run():
            core.zero_grad(set_to_none=True)
            H, hT, cT = f()
            (H.float().sum() + hT.float().sum() + cT.float().sum()).backward()
        return run

    def infer(f):
        def run():
            with torch.no_grad():
                f()
        return run

    fns = {}
    for name, f in (("loop", loop), ("fused", fused), ("scan", scan)):
        fns[name + " fwd+bwd"] = train(f)
        fns[name + " fwd-only"] = infer(f)

    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    with torch.no_grad():
        diff = (fused()[0].float() - loop()[0].float()).abs().max().item()
    emit("device: %s" % torch.cuda.get_device_name(0))
    emit("LSTM core hidden=%d T=%d B=%d input=%d bf16; max|H_fused - H_loop| = %.4f" % (Hd, T, B, I, diff))
    emit("%d warm-up + %d x %d timed calls each, the variants alternating" % (WARMUP, ROUNDS, ITERS))
    for fn in fns.values():
        timed(fn, WARMUP)
    times = {k: [] for k in fns}
    walls = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            per_call, wall = timed(fn, ITERS)
            times[k] += per_call
            walls[k].append(wall)
    med = {}
    for k in fns:
        q = statistics.quantiles(times[k], n=10)
        med[k] = statistics.median(times[k])
        emit("  %-15s device %9.1f us (p10-p90 %.1f-%.1f)   wall us per call, per round: %s"
             % (k, med[k], q[0], q[-1], " ".join("%.1f" % w for w in walls[k])))
    for mode in ("fwd+bwd", "fwd-only"):
        emit("  %s: loop/fused %.2fx, loop/scan %.2fx"
             % (mode, med["loop " + mode] / med["fused " + mode], med["loop " + mode] / med["scan " + mode]))

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
