"""IMPALA deep ResNet for Atari (Espeholt et al. 2018, "deep" variant).

Architecture parity with the reference model (examples/atari/models.py:9-153)
— this exact config is what BASELINE.json's headline benchmark names:
3 blocks of (3x3 conv -> 3x3/2 maxpool -> 2 residual blocks) with 16/32/32
channels, FC 3872->256, one-hot prev action + clipped reward appended,
optional LSTM(256), policy + baseline heads, multinomial sampling inside
forward.

MI355X notes: compute is bf16 (autocast over fp32 master weights, or bf16
shadow weights); the actor path is hipGraph-captured by the learner loop
(fixed [1, B] shapes), which removes the ~70-kernel launch overhead that
dominates small-CNN inference. Which kernels the trunk runs is decided per
call (the MOOLIB_AMD_* switches may change between two forwards):

| stage | condition | route |
|---|---|---|
| stem, conv1 | CUDA uint8 frames, bf16 compute, _kernels built, 4 input channels, not NO_CONV1_KERNEL | frames kernel (8-channel pad) + MFMA conv with the bias in the epilogue (`conv3x3.conv1_u8_autograd`; not subject to CONV3_KERNEL), then the section body with no pending bias |
| stem, frames kernel only | as above but other channel counts or NO_CONV1_KERNEL, and not NO_FRAMES_KERNEL | frames kernel, then section 0 as any other section |
| stem, eager | all else | `.to(dtype).mul_(1/255)`, channels_last on CUDA, then section 0 |
| section, fused | `fused_bias.available` | bias-free conv, pool, blocks through `forward_fused` with the conv bias pending |
| section, plain | otherwise | `nn.Conv2d`, pool, blocks as plain modules |
| block in `forward_fused` | no grad and `conv3x3.runs_on_mfma` | two fused MFMA conv launches |
| block in `forward_fused` | otherwise | `bias_relu`/relu, conv, `bias_relu`, conv, `bias_add2` |

A bias-free conv is the MFMA kernel when `conv3x3.runs_on_mfma`, else
F.conv2d (MIOpen). tests/test_trunk_routes.py pins the launches of each row.
"""
import os

import torch
import torch.nn.functional as F
from torch import nn

from moolib_amd.ops import act as act_ops
from moolib_amd.ops import conv3x3 as c3
from moolib_amd.ops import fused_bias
from moolib_amd.ops import lstm as lstm_ops
from moolib_amd.ops.fused_bias import bias_add2, bias_relu
from moolib_amd.ops.pool import maxpool3x3s2


def _conv3(x, conv):
    """Bias-free 3x3/s1/p1 conv: the MFMA kernel when the shape/dtype
    allows (forward AND input-gradient on the custom kernel — measured
    faster than MIOpen at every IMPALA shape, profiles/r2_conv3x3_micro),
    F.conv2d otherwise."""
    if c3.runs_on_mfma(x, conv.in_channels, conv.out_channels):
        return c3.conv3x3_autograd(x, conv)
    return F.conv2d(x, conv.weight, None, padding=1)


class ResidualBlock(nn.Module):
    def __init__(self, ch):
        super().__init__()
        self.conv0 = nn.Conv2d(ch, ch, 3, stride=1, padding=1)
        self.conv1 = nn.Conv2d(ch, ch, 3, stride=1, padding=1)

    def forward(self, x):
        y = self.conv0(F.relu(x))
        y = self.conv1(F.relu(y))
        return x + y

    def forward_fused(self, x, pending_bias=None):
        """Same math with the conv biases folded into the elementwise ops
        (ops/fused_bias): convs run bias-free, relu/add are one pass each.
        `pending_bias` is a per-channel bias the CALLER still owes `x`
        (section conv bias carried through the maxpool).

        Inference fast path (actor, no_grad): the whole block is TWO fused
        MFMA conv kernels (ops/conv3x3) — producer relu+bias on load,
        bias+residual on store.
        """
        ch = self.conv0.out_channels
        if not torch.is_grad_enabled() and c3.runs_on_mfma(x, x.size(1), ch):
            u = c3.conv3x3(
                x, c3.packed(self.conv0), ch,
                relu_in=True, bias_in=pending_bias,
            )
            return c3.conv3x3(
                u, c3.packed(self.conv1), ch,
                relu_in=True, bias_in=self.conv0.bias,
                epi=c3.EPI_BIAS_ADD, bias1=self.conv1.bias,
                res=x, bias2=pending_bias,
            )

        if pending_bias is not None:
            t = bias_relu(x, pending_bias)
        else:
            t = F.relu(x)
        u = _conv3(t, self.conv0)
        t = bias_relu(u, self.conv0.bias)
        u = _conv3(t, self.conv1)
        return bias_add2(u, self.conv1.bias, x, pending_bias)


class ConvSection(nn.Module):
    def __init__(self, in_ch, out_ch):
        super().__init__()
        self.conv = nn.Conv2d(in_ch, out_ch, 3, stride=1, padding=1)
        self.res0 = ResidualBlock(out_ch)
        self.res1 = ResidualBlock(out_ch)

    def forward(self, x):
        if fused_bias.available(x, self.conv.out_channels):
            # bias-free conv; per-channel bias commutes with the per-channel
            # spatial max, so it rides into res0 as a pending bias.
            return self.after_conv(_conv3(x, self.conv), self.conv.bias)
        return self.after_conv(self.conv(x), None)

    def after_conv(self, u, pending_bias):
        """Everything after the section conv: pool, res0, res1. `u` is the
        conv's output, short of `pending_bias` (a bias the conv left out)
        unless that is None."""
        u = maxpool3x3s2(u)
        if fused_bias.available(u):
            u = self.res0.forward_fused(u, pending_bias)
            return self.res1.forward_fused(u)
        assert pending_bias is None
        return self.res1(self.res0(u))


class AtariNet(nn.Module):
    def __init__(self, num_actions=18, input_channels=4, use_lstm=False):
        super().__init__()
        self.num_actions = num_actions
        self.use_lstm = use_lstm

        chans = [16, 32, 32]
        sections = []
        ch_in = input_channels
        for ch in chans:
            sections.append(ConvSection(ch_in, ch))
            ch_in = ch
        self.sections = nn.ModuleList(sections)

        self.fc = nn.Linear(3872, 256)
        core_in = self.fc.out_features + num_actions + 1
        if use_lstm:
            self.core = nn.LSTM(core_in, 256, num_layers=1)
            core_in = 256
        self.policy = nn.Linear(core_in, num_actions)
        self.baseline = nn.Linear(core_in, 1)
        # Optional dedicated RNG for the in-forward multinomial: hipGraph
        # replays of two captures racing on the DEFAULT generator's device
        # state is what forced the actor side stream off; per-capture
        # generators make concurrent replays sound.
        self.sample_generator = None
        # Optional [seed, step] state of ops.act (int64 [2] on the device):
        # when set, CUDA logits are sampled by the fused Philox head, one
        # launch and no torch generator at all.
        self.sampler_state = None

    def initial_state(self, batch_size=1):
        if not self.use_lstm:
            return tuple()
        return tuple(
            torch.zeros(self.core.num_layers, batch_size, self.core.hidden_size)
            for _ in range(2)
        )

    def stem(self, x):
        """Frames [N, C, 84, 84] (uint8 0..255) through section 0."""
        sec0 = self.sections[0]
        kernels = None
        if x.is_cuda and x.dtype == torch.uint8 and c3.bf16_compute(self.fc.weight):
            kernels = c3.kernels()
        if (
            kernels is not None
            and sec0.conv.in_channels == 4
            and not os.environ.get("MOOLIB_AMD_NO_CONV1_KERNEL")
        ):
            # uint8 frames -> conv1 + bias without a separate preprocessing
            # pass or a 19 MB fp intermediate. Under grad the same kernels
            # run through an autograd Function whose backward is our wgrad
            # kernel + a bias-sum — the first layer never touches MIOpen in
            # either direction.
            x = c3.conv1_u8_autograd(x, sec0.conv, 1.0 / 255.0)
            return sec0.after_conv(x, None)
        if kernels is not None and not os.environ.get("MOOLIB_AMD_NO_FRAMES_KERNEL"):
            x = kernels.frames_u8_to_bf16_nhwc(x, 1.0 / 255.0)
        else:
            x = x.to(self.fc.weight.dtype).mul_(1.0 / 255.0)
            if x.is_cuda:
                # NHWC: MIOpen's bf16 igemm kernels are NHWC-native; NCHW
                # input inserts a batched_transpose around every conv.
                # (Note: the FC input ordering then differs from the
                # CPU/NCHW path — a self-consistent permutation of learned
                # features.)
                x = x.contiguous(memory_format=torch.channels_last)
        return sec0(x)

    def forward(self, inputs, core_state=None):
        x = inputs["state"]
        reward = inputs["reward"]
        T, B = x.shape[:2]
        x = self.stem(x.flatten(0, 1))
        for s in self.sections[1:]:
            x = s(x)
        x = F.relu(x)
        x = x.reshape(T * B, -1)
        x = F.relu(self.fc(x))

        prev_action_onehot = F.one_hot(
            inputs["prev_action"].view(T * B).to(torch.int64), self.num_actions
        ).to(x.dtype)
        clipped_reward = reward.view(T * B, 1).clamp(-1, 1).to(x.dtype)
        core_input = torch.cat([x, clipped_reward, prev_action_onehot], dim=-1)

        if self.use_lstm:
            done = inputs["done"]
            core_input = core_input.view(T, B, -1)
            if lstm_ops.available(self.core.hidden_size, core_input.device) and (
                torch.is_autocast_enabled() or core_input.dtype == torch.bfloat16
            ):
                # fused MFMA sequence scan: one GEMM for x@W_ih over all T,
                # one kernel for the masked recurrence (fwd and bwd each).
                Xg = F.linear(
                    core_input.reshape(T * B, -1),
                    self.core.weight_ih_l0,
                    self.core.bias_ih_l0 + self.core.bias_hh_l0,
                ).view(T, B, -1).to(torch.bfloat16)
                notdone_f = (~done).float()
                h0 = core_state[0][0].to(torch.bfloat16)
                c0 = core_state[1][0].float()
                H, hT, cT = lstm_ops.fused_lstm_scan(
                    Xg, notdone_f, h0, c0, self.core.weight_hh_l0
                )
                core_output = H.flatten(0, 1)
                core_state = (
                    hT.unsqueeze(0).to(core_state[0].dtype),
                    cT.unsqueeze(0).to(core_state[1].dtype),
                )
            else:
                notdone = (~done).to(core_input.dtype)
                outputs = []
                for t in range(T):
                    nd = notdone[t].view(1, -1, 1)
                    core_state = tuple(nd * s for s in core_state)
                    out_t, core_state = self.core(core_input[t : t + 1], core_state)
                    outputs.append(out_t)
                core_output = torch.cat(outputs).flatten(0, 1)
        else:
            core_output = core_input

        policy_logits = self.policy(core_output).float()
        baseline = self.baseline(core_output).float()
        out = dict(
            policy_logits=policy_logits.view(T, B, self.num_actions),
            baseline=baseline.view(T, B),
        )
        if not torch.is_grad_enabled():
            # Actor path: sample the action in-forward (reference
            # models.py:134-140). The learner discards the sample (it
            # trains on the ACTOR's actions), and multinomial is one of
            # the slowest ops in the step (~230 us CPU+GPU at [672, 18]) —
            # skip it whenever autograd is recording.
            if self.sampler_state is not None and policy_logits.is_cuda:
                action = act_ops.sample_categorical(
                    policy_logits.view(T * B, self.num_actions), state=self.sampler_state
                )
            else:
                action = torch.multinomial(
                    F.softmax(policy_logits, dim=-1), num_samples=1,
                    generator=self.sample_generator,
                )
            out["action"] = action.view(T, B)
        return out, core_state


def create_model(num_actions=18, use_lstm=False, device="cpu"):
    model = AtariNet(num_actions=num_actions, use_lstm=use_lstm)
    model.to(device)
    return model
