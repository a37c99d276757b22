"""R2D2 on the HBM-resident prioritized replay: actor -> replay -> learner.

The same three peers as examples/r2d2_replay.py (a ReplayBuffer served over
the moolib RPC plane, an actor streaming LSTM rollouts into it, a learner
sampling prioritized batches), with a real learner: every environment's
sequence is one replay item that carries the recurrent state at its start,
the learner (moolib_amd.r2d2.R2D2Learner) computes n-step double-Q TD errors
with the fused gfx950 loss kernel, and the sequence priorities it returns are
what goes back into the buffer. On one node, `--ipc` serves samples as hipIpc
handles (zero-copy GPU->GPU).

With `--sumtree` the buffer is a SumTreeReplayBuffer (device-side sum tree,
stratified sampling): every unroll goes in with ONE add_batch(batch_dim=1),
straight from the device when the buffer lives on the GPU, and samples come
back time-major, so the learner needs no transposed views.

With `--fused-act` the actor's head is the fused epsilon-greedy kernel
(ops.act), and each of the `num_envs` environments explores at its own
epsilon of the Ape-X ladder.

With `--period N` the sequences overlap: one starts every N steps (R2D2 uses
half the unroll), each with the recurrent state at its own start. With
`--actor-priorities` every new sequence enters the buffer at the n-step TD
priority the actor computes from its own Q-values (ops.r2d2.actor_priorities,
one launch), not at the highest priority seen. Either flag routes the actor
through moolib_amd.r2d2.SequenceBuilder.

Run:  python examples/r2d2.py [--device cuda:0] [--ipc] [--sumtree] [--fused-act]
                              [--period 20] [--actor-priorities] [--seconds 20]
"""
import argparse
import time

import torch

import moolib_amd
from moolib_amd.envs import SyntheticAtariEnv
from moolib_amd.models.atari import AtariNet
from moolib_amd.ops.act import epsilon_ladder
from moolib_amd.r2d2 import R2D2Config, R2D2Learner
from moolib_amd.replay import ReplayBuffer, SumTreeReplayBuffer
from moolib_amd.utils import nest

SEQUENCE_KEYS = ("state", "reward", "done", "prev_action", "action")


def _add_sequences(buf, actor_rpc, sumtree, items, priorities):
    """Feed what a SequenceBuilder emitted ([T, B, ...] leaves, core_h / core_c
    [1, B, H], priorities [B] or None) to the replay; returns the RPC futures."""
    if sumtree:
        if buf.device.type == "cuda":  # same process, same GPU: no CPU detour
            buf.add_batch(items, priorities, batch_dim=1)
            return []
        return [actor_rpc.async_("replay_server", "replay.add_batch", items, priorities, 1)]
    seq = nest.map(lambda t: t.cpu(), items)
    priorities = None if priorities is None else priorities.cpu().tolist()
    futures = []
    for e in range(seq["reward"].shape[1]):
        item = {k: seq[k][:, e].contiguous() for k in SEQUENCE_KEYS + ("core_h", "core_c")}
        futures.append(actor_rpc.async_(
            "replay_server", "replay.add", item, None if priorities is None else priorities[e]
        ))
    return futures


def run(device=None, capacity=2048, unroll=40, burn_in=10, batch_size=16, num_envs=32,
        seconds=20.0, ipc=False, min_replay=None, sumtree=False, fused_act=False,
        period=None, actor_priorities=False):
    """Run the workload; returns a metrics dict."""
    device = device or ("cuda:0" if torch.cuda.is_available() else "cpu")
    ipc = bool(ipc and str(device).startswith("cuda"))
    min_replay = batch_size if min_replay is None else min_replay

    # Replay server peer: sequences live in HBM.
    server_rpc = moolib_amd.Rpc()
    server_rpc.set_name("replay_server")
    addr = [a for a in server_rpc.listen("127.0.0.1:0") if a.startswith("tcp://127")][0]
    buffer_cls = SumTreeReplayBuffer if sumtree else ReplayBuffer
    buf = buffer_cls(capacity, device=device, alpha=0.9, beta=0.6)
    buf.serve(server_rpc, "replay")

    envs = moolib_amd.EnvPool(
        lambda: SyntheticAtariEnv(num_actions=18),
        num_processes=4,
        batch_size=num_envs,
        num_batches=1,
    )
    learner = R2D2Learner(
        AtariNet(num_actions=18, use_lstm=True),
        R2D2Config(burn_in=burn_in, epsilon=0.05, fused_act=fused_act),
        device,
    )
    # the Ape-X ladder: every environment explores at its own rate
    epsilon = epsilon_ladder(num_envs).to(device) if fused_act else None
    actor_rpc = moolib_amd.Rpc()
    actor_rpc.set_name("actor")
    actor_rpc.set_timeout(30)
    actor_rpc.connect(addr)

    learner_rpc = moolib_amd.Rpc()
    learner_rpc.set_name("learner")
    learner_rpc.set_timeout(30)
    learner_rpc.connect(addr)

    # overlapping sequences and actor-side priorities go through a SequenceBuilder
    builder = None
    if period is not None or actor_priorities:
        builder = learner.sequence_builder(unroll, period)
    time_batcher = moolib_amd.Batcher(unroll, device) if builder is None else None
    core_state = tuple(s.to(device) for s in learner.online.initial_state(batch_size=num_envs))
    start_state = core_state  # recurrent state at the start of the current unroll
    prev_action = torch.zeros(num_envs, dtype=torch.int64, device=device)

    t0 = time.time()
    frames = sampled = learn_steps = 0
    add_futures = []
    metrics = None
    priority_sum, priority_count = 0.0, 0  # of the actor's initial priorities
    while time.time() - t0 < seconds:
        # ---- act (epsilon-greedy on the dueling Q-values) ----
        obs = envs.step(0, prev_action).result()
        dev = {k: t.to(device, copy=True) for k, t in obs.items()}
        dev["prev_action"] = prev_action
        inputs = {k: dev[k].unsqueeze(0) for k in ("state", "reward", "done", "prev_action")}
        if builder is None:
            action, core_state = learner.act(inputs, core_state, epsilon=epsilon)
            action = action.squeeze(0)
            frames += num_envs
            time_batcher.stack(dict(
                state=dev["state"], reward=dev["reward"], done=dev["done"],
                prev_action=prev_action, action=action,
            ))
        else:
            before = core_state  # what the network held when it consumed this step
            action, core_state, q = learner.act(
                inputs, core_state, epsilon=epsilon, return_q=True
            )
            action = action.squeeze(0)
            frames += num_envs
            emitted = builder.append(
                dict(state=dev["state"], reward=dev["reward"], done=dev["done"],
                     prev_action=prev_action, action=action),
                before, *(q if actor_priorities else (None, None)),
            )
        prev_action = action

        # ---- feed replay: one item per environment sequence ----
        if builder is not None:
            if emitted is not None:
                items, priorities = emitted
                if priorities is not None:
                    priority_sum += priorities.sum()
                    priority_count += num_envs
                add_futures += _add_sequences(buf, actor_rpc, sumtree, items, priorities)
        elif sumtree and not time_batcher.empty():
            # the whole [T, B, ...] unroll and its [1, B, H] start state, as they are
            items = dict(time_batcher.get())
            items = {k: items[k] for k in SEQUENCE_KEYS}
            items["core_h"], items["core_c"] = start_state
            if buf.device.type == "cuda":  # same process, same GPU: no CPU detour
                buf.add_batch(items, batch_dim=1)
            else:
                add_futures.append(
                    actor_rpc.async_("replay_server", "replay.add_batch", items, None, 1)
                )
            start_state = core_state
        elif not time_batcher.empty():
            seq = nest.map(lambda t: t.cpu(), time_batcher.get())  # [T, B, ...]
            h0, c0 = (s.cpu() for s in start_state)  # [1, B, H]
            for e in range(num_envs):
                item = {k: seq[k][:, e].contiguous() for k in SEQUENCE_KEYS}
                item["core_h"] = h0[:, e].contiguous()
                item["core_c"] = c0[:, e].contiguous()
                add_futures.append(actor_rpc.async_("replay_server", "replay.add", item))
            start_state = core_state
        add_futures = [f for f in add_futures if not f.done()]

        # ---- learner: prioritized sample, R2D2 step, true TD priorities back ----
        if len(buf) >= min_replay:
            fn = "replay.sample_ipc" if ipc else "replay.sample"
            if sumtree:  # time-major from the buffer: [T, B, ...] and [1, B, H]
                items, idx, w = learner_rpc.sync("replay_server", fn, batch_size, True)
                batch = {k: items[k] for k in SEQUENCE_KEYS}
                batch["core_state"] = (items["core_h"], items["core_c"])
            else:
                items, idx, w = learner_rpc.sync("replay_server", fn, batch_size)
                batch = {k: items[k].transpose(0, 1) for k in SEQUENCE_KEYS}  # time-major views
                batch["core_state"] = (
                    items["core_h"].transpose(0, 1), items["core_c"].transpose(0, 1)
                )
            metrics, priorities = learner.learn(batch, w)
            learner_rpc.sync("replay_server", "replay.update_priorities", idx, priorities.cpu())
            sampled += batch_size
            learn_steps += 1

    dt = time.time() - t0
    for f in add_futures:
        f.result()
    result = {
        "seconds": dt,
        "frames_acted": frames,
        "frames_per_s": frames / dt,
        "buffer_seqs": len(buf),
        "capacity": capacity,
        "sampled": sampled,
        "sampled_per_s": sampled / dt,
        "learn_steps": learn_steps,
        "mean_abs_td": float(metrics["mean_abs_td"]) if metrics else float("nan"),
        "loss": float(metrics["loss"]) if metrics else float("nan"),
        "unroll": unroll,
        "burn_in": burn_in,
        "batch_size": batch_size,
        "num_envs": num_envs,
        "ipc": ipc,
        "sumtree": bool(sumtree),
        "fused_act": bool(fused_act),
        "device": str(device),
    }
    if builder is not None:
        result["period"] = builder.period
        result["actor_priorities"] = bool(actor_priorities)
        result["initial_priority_mean"] = (
            float(priority_sum) / priority_count if priority_count else float("nan")
        )
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default=None)
    ap.add_argument("--capacity", type=int, default=2048)
    ap.add_argument("--unroll", type=int, default=40)
    ap.add_argument("--burn-in", type=int, default=10)
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--num-envs", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--ipc", action="store_true", help="serve samples as hipIpc handles")
    ap.add_argument("--sumtree", action="store_true",
                    help="SumTreeReplayBuffer: batched adds, stratified time-major samples")
    ap.add_argument("--fused-act", action="store_true",
                    help="fused epsilon-greedy head, one epsilon_ladder epsilon per environment")
    ap.add_argument("--period", type=int, default=None,
                    help="start a sequence every N steps (overlapping sequences); default: unroll")
    ap.add_argument("--actor-priorities", action="store_true",
                    help="new sequences enter at the actor's own n-step TD priority")
    a = ap.parse_args()
    m = run(a.device, a.capacity, a.unroll, a.burn_in, a.batch_size, a.num_envs, a.seconds,
            a.ipc, sumtree=a.sumtree, fused_act=a.fused_act, period=a.period,
            actor_priorities=a.actor_priorities)
    print(
        "r2d2: %.1fs, %d frames acted (%.0f/s), buffer %d/%d seqs, %d learner steps, "
        "%d sequences sampled (%.0f/s), mean |TD| %.4f, loss %.4f"
        % (
            m["seconds"], m["frames_acted"], m["frames_per_s"], m["buffer_seqs"],
            m["capacity"], m["learn_steps"], m["sampled"], m["sampled_per_s"],
            m["mean_abs_td"], m["loss"],
        )
    )
    if "initial_priority_mean" in m:
        print("r2d2: period %d, mean initial priority %.4f"
              % (m["period"], m["initial_priority_mean"]))


if __name__ == "__main__":
    main()
