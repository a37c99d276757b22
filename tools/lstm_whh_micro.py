#!/usr/bin/env python
"""Micro-timing of what the LSTM core does around weight_hh_l0 outside the
scan kernels, eager torch against hip/lstm_whh.hip.inc:

  grad   the backward's dW_hh. eager: cat([h0, H[:-1]]) * notdone, the fp32
         casts of dG and of that product, and the fp32 matmul, as
         _FusedLSTMScan.backward runs them; native: ops.lstm.recurrent_weight_grad
         (the MFMA kernel and, with more than one slab, the reduce).
  pack   the fp32 weight to both packed layouts. eager: .to(bf16), .t().contiguous()
         and the two pack_mfma_b, as forward plus backward run them; native:
         ops.lstm.pack_whh, one launch.

Shapes: T=80 B=64 H=512 (R2D2 learner, M=5120) and T=20 B=32 H=256 (IMPALA
learner, M=640). After a warm-up every call is bracketed by device events and
a round ends in a device synchronise; the two routes alternate over the
rounds. Reported: median and p10-p90 of the per-call device time, and the
largest difference between the routes' results on the same seeded inputs
(dW: fp32 sums in another order; pack: must be 0). Nothing is asserted.

Run on an MI355X:  python tools/lstm_whh_micro.py   (writes profiles/lstm_whh_micro.txt)
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from moolib_amd import _kernels  # noqa: F401  (no kernel, no measurement)
from moolib_amd.ops.lstm import pack_mfma_b, pack_whh, recurrent_weight_grad

WARMUP, ITERS, ROUNDS = 10, 20, 5
SHAPES = [("R2D2 learner", 80, 64, 512), ("IMPALA learner", 20, 32, 256)]


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


def eager_grad(dG, H, h0, notdone):
    T, B, _ = dG.shape
    Hm = torch.cat([h0.unsqueeze(0), H[:-1]]) * notdone.unsqueeze(-1).to(H.dtype)
    return dG.reshape(T * B, -1).t().float() @ Hm.reshape(T * B, -1).float()


def eager_pack(w_hh):
    w = w_hh.detach().to(torch.bfloat16)
    return pack_mfma_b(w.t().contiguous()), pack_mfma_b(w.contiguous())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstm_whh_micro.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lstm_whh_micro: needs a GPU; a CPU timing says nothing about it")

    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    emit("device: %s" % torch.cuda.get_device_name(0))
    emit("%d warm-up + %d x %d timed calls each, the routes alternating; device us, median (p10-p90)"
         % (WARMUP, ROUNDS, ITERS))
    for name, T, B, H in SHAPES:
        torch.manual_seed(0)
        bf = lambda *s: torch.randn(*s, device="cuda").to(torch.bfloat16)
        dG, Hs, h0 = bf(T, B, 4 * H), bf(T, B, H), bf(B, H)
        notdone = (torch.rand(T, B, device="cuda") > 0.1).float()
        w = torch.randn(4 * H, H, device="cuda") * 0.05
        fns = {
            ("grad", "eager"): lambda: eager_grad(dG, Hs, h0, notdone),
            ("grad", "native"): lambda: recurrent_weight_grad(dG, Hs, h0, notdone),
            ("pack", "eager"): lambda: eager_pack(w),
            ("pack", "native"): lambda: pack_whh(w),
        }
        ref = fns["grad", "eager"]()
        ddw = (fns["grad", "native"]() - ref).abs().max().item()
        dpack = max((a.float() - b.float()).abs().max().item()
                    for a, b in zip(fns["pack", "native"](), fns["pack", "eager"]()))
        for fn in fns.values():
            timed(fn, WARMUP)
        times = {k: [] for k in fns}
        for _ in range(ROUNDS):
            for k, fn in fns.items():
                times[k] += timed(fn, ITERS)
        emit("%s: T=%d B=%d (M=%d) H=%d; max|dW_native - dW_eager| = %.3g of max|dW| %.3g; "
             "max|pack_native - pack_eager| = %g"
             % (name, T, B, T * B, H, ddw, ref.abs().max().item(), dpack))
        for part in ("grad", "pack"):
            cells = []
            for route in ("eager", "native"):
                q = statistics.quantiles(times[part, route], n=10)
                cells.append("%s %8.1f (%.1f-%.1f)"
                             % (route, statistics.median(times[part, route]), q[0], q[-1]))
            ratio = (statistics.median(times[part, "eager"])
                     / statistics.median(times[part, "native"]))
            emit("  %-5s %s   eager/native %.2fx" % (part, "   ".join(cells), ratio))

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
