#!/usr/bin/env python
"""Microbenchmark: the one-launch actor section against the five launches it
replaces (pool kernel + two MFMA convs per residual block), at the actor's
batch and the three section shapes.

Device time, not enqueue time: each variant is captured into a hipGraph of
CALLS back-to-back calls (as the actor forward is replayed in training) and a
replay is timed between two device events. The variants alternate, round by
round, and the median round is reported with the min and max. There is no
preset ratio: the five-launch figure of the same run is the yardstick. Outputs
of the two variants are checked `torch.equal` before timing. Run on an MI355X:
    python tools/actor_section_micro.py            # writes profiles/actor_section_micro.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch
import torch.nn.functional as F

from moolib_amd.models.atari import ResidualBlock
from moolib_amd.ops import conv3x3 as c3
from moolib_amd.ops.pool import maxpool3x3s2

CALLS = 20    # calls per timed graph replay
ROUNDS = 30   # alternating rounds per variant

# (K, H, W, pending bias, relu_out) of sections 0, 1, 2 of the Atari trunk
SECTIONS = [(16, 84, 84, False, False), (32, 42, 42, True, False), (32, 21, 21, True, True)]


def five_launches(u, pending, res0, res1, relu_out):
    x = res1.forward_fused(res0.forward_fused(maxpool3x3s2(u), pending))
    return F.relu(x) if relu_out else x


def graph_of(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(CALLS):
            out = fn()
    g.replay()
    torch.cuda.synchronize()
    return g, out


def replay_us(g):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    g.replay()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1000.0 / CALLS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "actor_section_micro.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: this tool reports device time"
    torch.manual_seed(0)
    N = args.batch
    lines = [
        "actor section micro: device us per call, median [min..max] of %d alternating rounds, "
        "%d calls per graph replay, N=%d (%s)" % (ROUNDS, CALLS, N, torch.cuda.get_device_name(0)),
        "%-22s %26s %26s %8s  %s" % ("u [N,K,H,W]", "five launches (+relu)", "actor_section",
                                      "ratio", "MB moved / floor us at 8 TB/s"),
    ]
    with torch.no_grad():
        for K, H, W, with_pending, relu_out in SECTIONS:
            res0, res1 = (ResidualBlock(K).cuda().to(torch.bfloat16) for _ in range(2))
            for blk in (res0, res1):
                for conv in (blk.conv0, blk.conv1):
                    conv.bias.normal_(0, 0.1)
            pending = (torch.randn(K, device="cuda") * 0.1).to(torch.bfloat16) if with_pending else None
            u = torch.randn(N, K, H, W, device="cuda").to(torch.bfloat16).contiguous(
                memory_format=torch.channels_last)
            assert c3.actor_section_available(u, K)
            g5, out5 = graph_of(lambda: five_launches(u, pending, res0, res1, relu_out))
            g1, out1 = graph_of(lambda: c3.actor_section(u, pending, res0, res1, relu_out))
            assert torch.equal(out5, out1), "variants disagree"
            t5, t1 = [], []
            for _ in range(ROUNDS):
                t5.append(replay_us(g5))
                t1.append(replay_us(g1))
            m5, m1 = statistics.median(t5), statistics.median(t1)
            # what the fused launch must move: u in, the pooled result out
            mb = (u.numel() + out1.numel()) * 2 / 1e6
            lines.append("%-22s %9.1f [%6.1f..%6.1f] %9.1f [%6.1f..%6.1f] %8.2f  %.1f / %.1f" % (
                "[%d,%d,%d,%d]" % (N, K, H, W), m5, min(t5), max(t5), m1, min(t1), max(t1),
                m5 / m1, mb, mb / 8.0))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
