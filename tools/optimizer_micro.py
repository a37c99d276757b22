#!/usr/bin/env python
"""Micro-timing of the learner's optimizer step: optim.FlatAdam (fused flat
step, two HIP launches) against the eager chain it replaces, on the same GPU,
in the same process, on the same seeded gradients, the variants alternating.

The eager step is what ImpalaPeer._opt_fn runs in bf16-shadow mode:
clip_grad_norm_, torch.optim.Adam(foreach=True, capturable=True) and the flat
fp32 -> bf16 shadow copy. It is timed uncaptured (what a learning-rate schedule
forces on the eager path) and inside a parallel.graphs.GraphedCall (the
constant-lr case); the fused step is timed both ways too. The layout is
AtariNet's parameter list, with and without the LSTM.

After a warm-up each call is bracketed by device events; a window of calls
ended by a device synchronise gives the wall time per call, which is what a
launch-bound chain costs the host. Reported: the median and the p10-p90 spread
of the per-call device times over all rounds, the wall time per call of every
round, and the device launches of one call of each path (torch.profiler).
Nothing is asserted.

Run on an MI355X:  python tools/optimizer_micro.py   (writes profiles/optimizer_micro.txt)
"""
import argparse
import copy
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from moolib_amd import _kernels  # noqa: F401  (no kernel, no measurement)
from moolib_amd.impala import flatten_master_shadow
from moolib_amd.models.atari import AtariNet
from moolib_amd.optim import FlatAdam
from moolib_amd.parallel.graphs import GraphedCall

WARMUP, ITERS, ROUNDS = 10, 50, 3
LR, BETAS, EPS, CLIP = 6e-4, (0.9, 0.999), 1e-8, 40.0


class Setup:
    """One master/shadow pair laid out as ImpalaPeer lays it out."""

    def __init__(self, use_lstm, fused):
        torch.manual_seed(0)
        self.model = AtariNet(num_actions=18, use_lstm=use_lstm).cuda()
        self.fwd = copy.deepcopy(self.model).to(torch.bfloat16)
        self.params = [p for p in self.model.parameters() if p.requires_grad]
        fwd_params = [p for p in self.fwd.parameters() if p.requires_grad]
        self.flat_master, self.flat_shadow, self.flat_grad32, _ = flatten_master_shadow(
            self.params, fwd_params
        )
        g = torch.Generator().manual_seed(1)
        self.flat_grad32.copy_(0.05 * torch.randn(self.flat_grad32.numel(), generator=g))
        if fused:
            self.opt = FlatAdam(
                self.params, lr=LR, betas=BETAS, eps=EPS, max_grad_norm=CLIP,
                flat=(self.flat_master, self.flat_grad32, self.flat_shadow),
            )
            self.step = self.fused_step
        else:
            self.opt = torch.optim.Adam(
                self.params, lr=LR, betas=BETAS, eps=EPS, foreach=True, capturable=True
            )
            self.step = self.eager_step

    def eager_step(self, _inputs=None):
        norm = torch.nn.utils.clip_grad_norm_(self.params, CLIP)
        self.opt.step()
        self.flat_shadow.copy_(self.flat_master, non_blocking=True)
        return norm

    def fused_step(self, _inputs=None):
        return self.opt.step()


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
        names = [
            e.name for e in prof.events()
            if e.device_type == torch.autograd.DeviceType.CUDA
            # the optimizer's record_function range shows up on the device
            # timeline too; it is no launch
            and not e.name.startswith("Optimizer.step#")
        ]
        if not names:
            return "n/a"
        if len(names) <= 4:  # few enough to name them
            return "%d (%s)" % (len(names), ", ".join(n.split("(")[0][-40:] for n in names))
        return str(len(names))
    except Exception as e:  # noqa: BLE001 — the count is a courtesy, the timing is the point
        return "n/a (%s)" % type(e).__name__


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optimizer_micro.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("optimizer_micro: needs a GPU; a CPU timing says nothing about it")
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    emit("device: %s" % torch.cuda.get_device_name(0))
    emit("us per optimizer step, %d warm-up + %d x %d timed calls each, the variants alternating"
         % (WARMUP, ROUNDS, ITERS))
    for use_lstm in (False, True):
        setups = {
            "eager": Setup(use_lstm, fused=False),
            "fused": Setup(use_lstm, fused=True),
            "eager_graph": Setup(use_lstm, fused=False),
            "fused_graph": Setup(use_lstm, fused=True),
        }
        fns = {}
        for k, s in setups.items():
            if k.endswith("_graph"):
                call = GraphedCall(s.step, warmup=3, name=k)
                fns[k] = (lambda c: lambda: c({}))(call)
                for _ in range(5):  # warm-up and capture
                    fns[k]()
                assert call.graph is not None and not call.failed, k + ": not captured"
            else:
                fns[k] = s.step
        n = setups["eager"].flat_master.numel()
        emit("launches per call: eager %s, fused %s (uncaptured, AtariNet use_lstm=%s)"
             % (launches(fns["eager"]), launches(fns["fused"]), use_lstm))
        compare("AtariNet use_lstm=%s: %d parameter tensors, N = %d"
                % (use_lstm, len(setups["eager"].params), n), fns, emit)
        del setups, fns
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
