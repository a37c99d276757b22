"""Deterministic probe for the rollout path (docs/ROLLOUT_TESTS.md):
ImpalaPeer.act_once -> time batcher -> learn batcher -> compute_gradients.

LedgerEnv writes what it was told into its observation and ProbeNet computes
small-integer outputs from exactly the inputs AtariNet conditions on, so a
learner batch can be checked against itself: re-running ProbeNet on the
batch's env_outputs and initial_core_state must reproduce the batch's
actor_outputs element for element. Every value is an integer of at most 256
in magnitude, exact in bf16 and fp32, so the same probe serves as the bf16
shadow model on the GPU and every comparison is `torch.equal`.

A plain helper module (like kernel_refs.py), used by
tests/test_rollout_integrity.py.
"""
import gc
import os
import time

import numpy as np
import torch
from torch import nn

import moolib_amd
from moolib_amd.impala import ImpalaConfig, ImpalaPeer
from moolib_amd.utils import nest

EPISODE_LEN = 7   # done is true on every 7th step of an env
AFTER_RESET = 255  # plane 1 of an observation that reset() produced


class LedgerEnv:
    """Observation uint8 [4, 2, 2], every plane constant over its 2x2:

    plane 0  step counter of the episode (0 after reset; stays below 200)
    plane 1  the action received by the step() that produced this
             observation, AFTER_RESET after reset()
    plane 2  episode index mod 200
    plane 3  a per-env salt, constant for the env's life. Envs of one
             worker process get consecutive salts, so the rows of a batch
             differ and a row mix-up between leaves cannot go unnoticed.

    reward = float(action); done on every EPISODE_LEN-th step. The pool
    resets on done and still reports that step's reward and done, so
    reward[t+1] == action[t] always, and plane 1 of state[t+1] equals
    action[t] wherever done[t+1] is false.
    """

    _created = 0  # per worker process (the pool creates envs after forking)

    def __init__(self):
        self.salt = (os.getpid() * 8 + LedgerEnv._created) % 200
        LedgerEnv._created += 1
        self.count = 0
        self.episode = -1

    def _obs(self, last_action):
        obs = np.empty((4, 2, 2), dtype=np.uint8)
        obs[0] = self.count % 200
        obs[1] = last_action
        obs[2] = self.episode % 200
        obs[3] = self.salt
        return obs

    def reset(self):
        self.count = 0
        self.episode += 1
        return self._obs(AFTER_RESET)

    def step(self, action):
        action = int(action)
        self.count += 1
        done = self.count >= EPISODE_LEN
        return self._obs(action), float(action), done, {}


class ProbeNet(nn.Module):
    """Stub with AtariNet's calling convention and integer outputs.

    policy_logits[t, b, a] = (counter + 2*prev_action + 3*clipped_reward
                              + 5*core + salt + a*(counter + 1)) % 11
    baseline[t, b]         = (counter + core) % 5
    action[t, b]           = (counter + prev_action + 1 + salt) % A
                             (no_grad only, like AtariNet; no sampling)

    counter and salt are planes 0 and 3 of the observation; clipped_reward
    is reward.clamp(-1, 1) as in AtariNet. With use_lstm the core state is
    (h, c), both [1, B, 1]; per step both are masked by ~done exactly as
    AtariNet's fallback loop does, then h += 1 and c += 2, and core = h + c
    (at most 3 * EPISODE_LEN). Without it core = 0.

    The one trainable parameter enters every output multiplied by zero:
    backward, the accumulator and Adam all run, the outputs never move.
    """

    def __init__(self, num_actions=6, use_lstm=False):
        super().__init__()
        self.num_actions = num_actions
        self.use_lstm = use_lstm
        self.w = nn.Parameter(torch.zeros(1))
        self.sample_generator = None

    def initial_state(self, batch_size=1):
        if not self.use_lstm:
            return tuple()
        return tuple(torch.zeros(1, batch_size, 1) for _ in range(2))

    def forward(self, inputs, core_state=None):
        state = inputs["state"]
        T, B = state.shape[:2]
        counter = state[:, :, 0, 0, 0].to(torch.int64)
        salt = state[:, :, 3, 0, 0].to(torch.int64)
        prev_action = inputs["prev_action"].view(T, B).to(torch.int64)
        clipped_reward = inputs["reward"].view(T, B).clamp(-1, 1).to(torch.int64)

        if self.use_lstm:
            h, c = core_state
            notdone = (~inputs["done"]).to(h.dtype)
            cores = []
            for t in range(T):
                nd = notdone[t].view(1, -1, 1)
                h = nd * h + 1
                c = nd * c + 2
                cores.append((h + c).view(B))
            core = torch.stack(cores).to(torch.int64)
            core_state = (h, c)
        else:
            core = torch.zeros_like(counter)

        a = torch.arange(self.num_actions, device=state.device).view(1, 1, -1)
        logits = (
            (counter + 2 * prev_action + 3 * clipped_reward + 5 * core + salt).unsqueeze(-1)
            + a * (counter + 1).unsqueeze(-1)
        ) % 11
        zero = (0 * self.w).float()
        out = dict(
            policy_logits=logits.float() + zero,
            baseline=((counter + core) % 5).float() + zero,
        )
        if not torch.is_grad_enabled():
            out["action"] = (counter + prev_action + 1 + salt) % self.num_actions
        return out, core_state


def make_broker():
    rpc = moolib_amd.Rpc()
    rpc.set_name("broker")
    broker = moolib_amd.Broker(rpc)
    addr = rpc.listen("127.0.0.1:0")[0]
    return broker, addr


def probe_config(addr, **kw):
    """The small config the rollout tests share; `kw` overrides."""
    base = dict(
        num_actions=6,
        actor_batch_size=4,
        num_actor_batches=2,
        num_actor_cpus=2,
        batch_size=4,
        unroll_length=5,
        virtual_batch_size=4,
        connect=addr,
        total_steps=1e6,
        seed=3,
    )
    base.update(kw)
    return ImpalaConfig(**base)


def make_probe_peer(**kw):
    """(peer, broker) with LedgerEnv and ProbeNet."""
    broker, addr = make_broker()
    cfg = probe_config(addr, **kw)
    model = ProbeNet(num_actions=cfg.num_actions, use_lstm=cfg.use_lstm)
    return ImpalaPeer(cfg, LedgerEnv, model=model, broker=broker), broker


def close_peer(peer):
    """Drop everything a peer owns (env workers, RPC threads, device
    buffers) so the next case starts from nothing. The handles have no
    close(); their destructors do the work once the references are gone."""
    for name in list(vars(peer)):
        setattr(peer, name, None)
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def collect_batches(peer, n, timeout=60.0):
    """Drive peer.step_once() until `n` learner batches have reached
    compute_gradients; return deep CPU copies of them, in order."""
    got = []
    inner = peer.compute_gradients

    def recording(data):
        if len(got) < n:
            got.append(
                nest.map(
                    lambda t: t.detach().clone().cpu() if isinstance(t, torch.Tensor) else t,
                    data,
                )
            )
        return inner(data)

    peer.compute_gradients = recording
    try:
        t0 = time.time()
        while len(got) < n and time.time() - t0 < timeout:
            peer.step_once()
    finally:
        del peer.compute_gradients  # back to the class's method
    assert len(got) == n, "only %d of %d learner batches within %.0fs" % (len(got), n, timeout)
    return got
