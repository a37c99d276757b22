#!/usr/bin/env python
"""Micro-timing of the policy and baseline heads, from the bf16 tensor the core
hands over:

  eager   what AtariNet runs with fused_heads=False: without an LSTM one_hot,
          clamp, cat, then policy(core).float() and baseline(core).float(); with
          one the two linears alone. fp32 weights run under autocast, which
          casts weights and biases to bf16 on every call; bf16 weights (shadow
          weights) run as they are.
  fused   ops.heads.policy_value_heads (hip/heads.hip.inc).

Shapes: M = 128 and 256 (actor), 672 (IMPALA learner, 21 x 32), 5120 (R2D2
learner, 80 x 64); composite mode with A = 18, dense mode with D = 256 and 512.
Each is timed forward-only under no_grad and forward+backward (fp32 gradients
into both outputs; gradients to x and the four parameters), as eager launches
and as one replay of a captured graph. After a warm-up every call is bracketed
by device events and a round ends in a device synchronise; the two routes
alternate over the rounds. Reported: median and p10-p90 of the per-call device
time, and the largest difference between the two routes' logits on the same
seeded inputs. --profile runs only the fused route a few times, uncaptured, for
a kernel trace that counts its launches. Nothing is asserted.

Run on an MI355X:  python tools/heads_micro.py   (writes profiles/heads_micro.txt)
"""
import argparse
import contextlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch
import torch.nn.functional as F

from moolib_amd import _kernels  # noqa: F401  (no kernel, no measurement)
from moolib_amd.ops.heads import policy_value_heads

WARMUP, ITERS, ROUNDS = 5, 10, 3
SHAPES = [("actor", 128), ("actor", 256), ("IMPALA learner", 672), ("R2D2 learner", 5120)]
MODES = [("composite", 256), ("dense", 256), ("dense", 512)]
A = 18
BF16 = torch.bfloat16


def eager_heads(x, policy, baseline, reward=None, prev_action=None):
    """The lines of AtariNet.forward with fused_heads=False."""
    if reward is not None:
        onehot = F.one_hot(prev_action.to(torch.int64), A).to(x.dtype)
        x = torch.cat([x, reward.view(-1, 1).clamp(-1, 1).to(x.dtype), onehot], dim=-1)
    return policy(x).float(), baseline(x).float().view(-1)


def fused_heads(x, policy, baseline, reward=None, prev_action=None):
    return policy_value_heads(x, policy.weight, policy.bias, baseline.weight, baseline.bias,
                              reward, prev_action)


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


def routes(M, mode, D, wdtype):
    """{(route, 'fwd' | 'fwd+bwd'): callable} on one set of seeded inputs."""
    torch.manual_seed(0)
    K = D + 1 + A if mode == "composite" else D
    policy = torch.nn.Linear(K, A).cuda().to(wdtype)
    baseline = torch.nn.Linear(K, 1).cuda().to(wdtype)
    x = torch.randn(M, D, device="cuda").to(BF16).requires_grad_()
    extra = ()
    if mode == "composite":
        extra = (torch.randn(M, device="cuda") * 2, torch.randint(0, A, (M,), device="cuda"))
    GL, GB = torch.randn(M, A, device="cuda"), torch.randn(M, device="cuda")
    amp = ((lambda: torch.autocast("cuda", dtype=BF16)) if wdtype == torch.float32
           else contextlib.nullcontext)
    fns = {}
    for rname, op in (("eager", eager_heads), ("fused", fused_heads)):
        def fwd(op=op):
            with torch.no_grad(), amp():
                return op(x, policy, baseline, *extra)

        def train(op=op):
            x.grad = None
            policy.zero_grad(set_to_none=True)
            baseline.zero_grad(set_to_none=True)
            with amp():
                logits, value = op(x, policy, baseline, *extra)
            torch.autograd.backward([logits, value], [GL, GB])

        fns[rname, "fwd"], fns[rname, "fwd+bwd"] = fwd, train
    return fns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heads_micro.txt"))
    ap.add_argument("--profile", action="store_true",
                    help="3 uncaptured forward+backward calls of the fused route at M=672, "
                         "composite, and nothing else: for a kernel trace")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("heads_micro: needs a GPU; a CPU timing says nothing about it")
    if args.profile:
        fn = routes(672, "composite", 256, torch.float32)["fused", "fwd+bwd"]
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        return

    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    emit("device: %s" % torch.cuda.get_device_name(0))
    emit("%d warm-up + %d x %d timed calls each, the routes alternating; device us, median (p10-p90)"
         % (WARMUP, ROUNDS, ITERS))
    for name, M in SHAPES:
        for mode, D in MODES:
            for wdtype in (torch.float32, BF16):
                base = routes(M, mode, D, wdtype)
                diff = (base["eager", "fwd"]()[0] - base["fused", "fwd"]()[0]).abs().max().item()
                fns = {k + ("launches",): fn for k, fn in base.items()}
                for k, fn in base.items():
                    fns[k + ("graph",)] = captured(fn)
                for fn in fns.values():
                    timed(fn, WARMUP)
                times = {k: [] for k in fns}
                for _ in range(ROUNDS):
                    for k, fn in fns.items():
                        times[k] += timed(fn, ITERS)
                emit("%s: M=%d %s D=%d A=%d weight %s; max|logits_fused - logits_eager| = %.4f"
                     % (name, M, mode, D, A, str(wdtype).replace("torch.", ""), diff))
                for how in ("launches", "graph"):
                    for what in ("fwd", "fwd+bwd"):
                        cells = []
                        for rname in ("eager", "fused"):
                            t = times[rname, what, how]
                            q = statistics.quantiles(t, n=10)
                            cells.append("%s %8.1f (%.1f-%.1f)"
                                         % (rname, statistics.median(t), q[0], q[-1]))
                        ratio = (statistics.median(times["eager", what, how])
                                 / statistics.median(times["fused", what, how]))
                        emit("  %-8s %-8s %s   eager/fused %.2fx"
                             % (how, what, "   ".join(cells), ratio))

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
