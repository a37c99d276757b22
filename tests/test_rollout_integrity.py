"""Contents of the learner batches, and of what the actor reads after the
weights change (docs/ROLLOUT_TESTS.md has the invariants and the findings).

The rollout path keeps persistent buffers with stable addresses so that
hipGraph replay works (prev_action, core_state, staged H2D buffers, packed
conv weights). Each is an aliasing hazard; these tests look at the values
that come out the far end:

* TestRolloutCpu / TestRolloutGpu: a deterministic env and a stub model
  (tests/rollout_probe.py) whose outputs are a pure integer function of the
  inputs AtariNet conditions on. Re-running the stub on a learner batch must
  reproduce the batch's actor outputs exactly; named invariants say what
  broke when it does not.
* TestWeightPropagation: after an eager optimizer step, graphed optimizer
  steps and a state sync, the actor (graph replay and eager) must compute
  what a fresh AtariNet built from the current master weights computes.
* TestGraphedCallGpu: the replay contract of parallel/graphs.GraphedCall.

All comparisons are `torch.equal`.
"""
import types

import pytest
import torch

import rollout_probe as P
from moolib_amd.impala import ImpalaPeer, flatten_master_shadow
from moolib_amd.parallel.graphs import GraphedCall

gpu = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")


# -------------------------------------------------------------- invariants
#
# Each takes the recorded learner batches (CPU copies, in learner order) and
# the peer's config. Leaves are [T+1, batch_size, ...]; initial_core_state
# leaves are [1, batch_size, 1].


def _first_unroll_rows(j, cfg):
    """Mask of the rows of learner batch j that are an env's FIRST unroll.

    Unrolls complete in env-batch order (0, 1, 0, 1, ...), each adds
    actor_batch_size rows to the learn batcher, and cat() keeps the order:
    row r of learner batch j is row j*batch_size + r of that stream, and the
    first num_actor_batches unrolls are the first ones."""
    g = j * cfg.batch_size + torch.arange(cfg.batch_size)
    return (g // cfg.actor_batch_size) < cfg.num_actor_batches


def _planes(batch):
    s = batch["env_outputs"]["state"]
    return [s[:, :, k, 0, 0].to(torch.int64) for k in range(4)]


def _eq(got, want, what, j):
    assert torch.equal(got, want), "%s, learner batch %d:\ngot  %s\nwant %s" % (
        what, j, got.tolist(), want.tolist())


def check_learner_reproduces_actor(batches, cfg):
    model = P.ProbeNet(num_actions=cfg.num_actions, use_lstm=cfg.use_lstm)
    for j, b in enumerate(batches):
        core = tuple(s.float() for s in b["initial_core_state"])
        with torch.no_grad():
            out, _ = model(b["env_outputs"], core)
        ao = b["actor_outputs"]
        _eq(ao["policy_logits"].float(), out["policy_logits"],
            "policy_logits recomputed from the batch differ from the actor's", j)
        _eq(ao["action"].to(torch.int64), out["action"],
            "action recomputed from the batch differs from the actor's", j)
        _eq(ao["baseline"].float(), out["baseline"],
            "baseline recomputed from the batch differs from the actor's", j)


def check_prev_action_is_previous_action(batches, cfg):
    for j, b in enumerate(batches):
        _eq(b["env_outputs"]["prev_action"][1:], b["actor_outputs"]["action"][:-1],
            "prev_action[t+1] != action[t]", j)


def check_first_prev_action_zero(batches, cfg):
    seen = 0
    for j, b in enumerate(batches):
        rows = _first_unroll_rows(j, cfg)
        seen += int(rows.sum())
        got = b["env_outputs"]["prev_action"][0][rows]
        _eq(got, torch.zeros_like(got), "prev_action[0] != 0 in a first unroll", j)
    assert seen == cfg.actor_batch_size * cfg.num_actor_batches, seen


def check_reward_is_previous_action(batches, cfg):
    for j, b in enumerate(batches):
        _eq(b["env_outputs"]["reward"][1:], b["actor_outputs"]["action"][:-1].float(),
            "reward[t+1] != action[t]", j)


def check_state_records_previous_action(batches, cfg):
    for j, b in enumerate(batches):
        plane1 = _planes(b)[1][1:]
        done = b["env_outputs"]["done"][1:]
        want = torch.where(
            done, torch.full_like(plane1, P.AFTER_RESET), b["actor_outputs"]["action"][:-1]
        )
        _eq(plane1, want, "plane 1 of state[t+1] != action[t] (255 where done)", j)


def check_counters(batches, cfg):
    for j, b in enumerate(batches):
        counter, _, episode, salt = _planes(b)
        done = b["env_outputs"]["done"][1:].to(torch.int64)
        _eq(counter[1:], (counter[:-1] + 1) * (1 - done),
            "step counter does not advance by 1 / restart on done", j)
        _eq(episode[1:], (episode[:-1] + done) % 200,
            "episode index does not advance exactly on done", j)
        _eq(salt[1:], salt[:-1], "rows changed env inside an unroll", j)
        _eq(done, (counter[:-1] == P.EPISODE_LEN - 1).to(torch.int64),
            "done is not every %d-th step" % P.EPISODE_LEN, j)


def check_first_initial_core_state_zero(batches, cfg):
    for j, b in enumerate(batches):
        core = b["initial_core_state"]
        assert len(core) == (2 if cfg.use_lstm else 0), (j, len(core))
        rows = _first_unroll_rows(j, cfg)
        for s in core:
            got = s.float()[0, rows, 0]
            _eq(got, torch.zeros_like(got),
                "initial_core_state of a first unroll is not zero", j)


def check_unroll_overlap(batches, cfg):
    """With batch_size == actor_batch_size learner batch j is unroll
    j // num_actor_batches of env batch j % num_actor_batches, rows in
    place: entry 0 of the next unroll is entry T of this one."""
    assert cfg.batch_size == cfg.actor_batch_size
    nb = cfg.num_actor_batches
    pairs = 0
    for j in range(len(batches) - nb):
        a, b = batches[j], batches[j + nb]
        for group in ("env_outputs", "actor_outputs"):
            for k in a[group]:
                _eq(b[group][k][0], a[group][k][-1],
                    "%s[%s]: entry 0 of the next unroll != entry T" % (group, k), j)
        pairs += 1
    assert pairs >= 2, pairs


def check_not_vacuous(batches, cfg):
    assert len(batches) >= 6
    assert any(bool(b["env_outputs"]["done"].any()) for b in batches), "no done"
    actions = torch.cat([b["actor_outputs"]["action"].flatten() for b in batches])
    assert actions.unique().numel() >= 2, actions.unique().tolist()
    salts = torch.cat([_planes(b)[3].flatten() for b in batches])
    assert salts.unique().numel() >= 2, salts.unique().tolist()
    for b in batches:
        assert b["env_outputs"]["state"].shape[:2] == (cfg.unroll_length + 1, cfg.batch_size)


ROW_CHECKS = [
    check_not_vacuous,
    check_learner_reproduces_actor,
    check_prev_action_is_previous_action,
    check_first_prev_action_zero,
    check_reward_is_previous_action,
    check_state_records_previous_action,
    check_counters,
    check_first_initial_core_state_zero,
]


# --------------------------------------------------------------------- CPU

CPU_CASES = [
    # (use_lstm, batch_size, learner batches to record)
    (False, 4, 6),
    (True, 4, 6),
    # batch_size 3 against actor batches of 4: cat() splits every unroll
    # across learner batches and rows of both env batches share a batch
    (True, 3, 8),
]


@pytest.fixture(scope="class", params=CPU_CASES, ids=lambda c: "lstm%d-bs%d" % (c[0], c[1]))
def cpu_rollout(request):
    use_lstm, batch_size, n = request.param
    peer, broker = P.make_probe_peer(
        device="cpu", autocast_bf16=False, use_lstm=use_lstm,
        batch_size=batch_size, virtual_batch_size=batch_size,
    )
    try:
        cfg = peer.cfg
        batches = P.collect_batches(peer, n)
    finally:
        P.close_peer(peer)
        del broker
    return batches, cfg


@pytest.mark.timeout(300)
class TestRolloutCpu:
    """device="cpu": T=5, two env batches of 4."""

    def test_not_vacuous(self, cpu_rollout):
        check_not_vacuous(*cpu_rollout)

    def test_learner_reproduces_actor(self, cpu_rollout):
        check_learner_reproduces_actor(*cpu_rollout)

    def test_prev_action_is_previous_action(self, cpu_rollout):
        check_prev_action_is_previous_action(*cpu_rollout)

    def test_first_prev_action_zero(self, cpu_rollout):
        check_first_prev_action_zero(*cpu_rollout)

    def test_reward_is_previous_action(self, cpu_rollout):
        check_reward_is_previous_action(*cpu_rollout)

    def test_state_records_previous_action(self, cpu_rollout):
        check_state_records_previous_action(*cpu_rollout)

    def test_counters(self, cpu_rollout):
        check_counters(*cpu_rollout)

    def test_first_initial_core_state_zero(self, cpu_rollout):
        check_first_initial_core_state_zero(*cpu_rollout)

    def test_unroll_overlap(self, cpu_rollout):
        batches, cfg = cpu_rollout
        if cfg.batch_size != cfg.actor_batch_size:
            # rows are not in place; the other checks cover this case
            return
        check_unroll_overlap(batches, cfg)


class TestProbeSelfCheck:
    """The probe itself, without a peer: it must be able to tell the two
    aliasing bugs from a correct rollout."""

    def _rollout(self, T=12, B=3, alias_prev_action=False):
        envs = [P.LedgerEnv() for _ in range(B)]
        model = P.ProbeNet(num_actions=6, use_lstm=True)
        core = model.initial_state(B)
        initial_core = core
        prev_action = torch.zeros(B, dtype=torch.int64)
        obs = [e.reset() for e in envs]
        reward, done = [0.0] * B, [False] * B
        eo = {k: [] for k in ("state", "reward", "done", "prev_action")}
        ao = {k: [] for k in ("policy_logits", "baseline", "action")}
        import numpy as np

        for _ in range(T):
            step = {
                "state": torch.from_numpy(np.stack(obs)),
                "reward": torch.tensor(reward),
                "done": torch.tensor(done),
                "prev_action": prev_action,
            }
            with torch.no_grad():
                out, core = model({k: v.unsqueeze(0) for k, v in step.items()}, core)
            action = out["action"][0]
            if alias_prev_action:
                step["prev_action"] = action
            for k in eo:
                eo[k].append(step[k])
            for k in ao:
                ao[k].append(out[k][0])
            prev_action = action
            for i, e in enumerate(envs):
                o, r, d, _ = e.step(int(action[i]))
                obs[i], reward[i], done[i] = (e.reset() if d else o), r, d
        return {
            "env_outputs": {k: torch.stack(v) for k, v in eo.items()},
            "actor_outputs": {k: torch.stack(v) for k, v in ao.items()},
            "initial_core_state": initial_core,
        }, core

    def _cfg(self, T, B):
        return P.probe_config(
            "", unroll_length=T - 1, actor_batch_size=B, batch_size=B,
            num_actor_batches=1, use_lstm=True, device="cpu",
        )

    def test_correct_rollout_passes(self):
        batch, _ = self._rollout()
        cfg = self._cfg(12, 3)
        for check in ROW_CHECKS[1:]:
            check([batch], cfg)
        assert batch["env_outputs"]["done"].any()
        assert batch["actor_outputs"]["action"].unique().numel() >= 2

    def test_aliased_prev_action_is_caught(self):
        batch, _ = self._rollout(alias_prev_action=True)
        cfg = self._cfg(12, 3)
        with pytest.raises(AssertionError, match="policy_logits recomputed"):
            check_learner_reproduces_actor([batch], cfg)
        with pytest.raises(AssertionError, match="prev_action"):
            check_prev_action_is_previous_action([batch], cfg)

    def test_aliased_initial_core_state_is_caught(self):
        batch, final_core = self._rollout()
        batch["initial_core_state"] = final_core
        cfg = self._cfg(12, 3)
        with pytest.raises(AssertionError, match="policy_logits recomputed"):
            check_learner_reproduces_actor([batch], cfg)
        with pytest.raises(AssertionError, match="initial_core_state"):
            check_first_initial_core_state_zero([batch], cfg)

    def test_values_exact_in_bf16(self):
        batch, core = self._rollout(T=30)
        for t in list(batch["actor_outputs"].values()) + list(core):
            f = t.float()
            assert torch.equal(f.to(torch.bfloat16).float(), f)
            assert f.abs().max() <= 256


# --------------------------------------------------------------------- GPU

GPU_CASES = [
    # (prefetch_h2d, pinned_staging, graph_actor, bf16_weights)
    (True, True, True, True),
    (True, True, False, True),
    (False, True, True, True),
    (False, True, False, True),
    (False, False, True, True),
    (False, False, False, True),
    (True, True, True, False),
    (True, True, False, False),
]


def _gpu_id(c):
    staging = "prefetch" if c[0] else ("pinned" if c[1] else "pageable")
    return "%s-%s-%s" % (staging, "graph" if c[2] else "eager", "bf16w" if c[3] else "fp32w")


@gpu
@requires_gpu
class TestRolloutGpu:
    """Peer on cuda, T=3, B=4, use_lstm: every staging mode with the actor
    graph on and off."""

    @pytest.mark.timeout(120)
    @pytest.mark.parametrize("case", GPU_CASES, ids=_gpu_id)
    def test_learner_batches(self, case):
        prefetch, pinned, graph_actor, bf16_weights = case
        peer, broker = P.make_probe_peer(
            device="cuda:0", use_lstm=True, unroll_length=3,
            prefetch_h2d=prefetch, pinned_staging=pinned,
            graph_actor=graph_actor, bf16_weights=bf16_weights,
        )
        try:
            cfg = peer.cfg
            assert cfg.prewarm and not cfg.graph_learner and not cfg.actor_side_stream
            assert peer.bf16_shadow == bf16_weights
            batches = P.collect_batches(peer, 8)
            # the mode under test really ran: no silent fallback
            if graph_actor:
                assert isinstance(peer._actor_call, GraphedCall)
                assert peer._actor_call.graph is not None and not peer._actor_call.failed
                assert peer._actor_call.calls >= peer._actor_call.warmup
            else:
                assert not isinstance(peer._actor_call, GraphedCall)
            staged = any(st.staged is not None for st in peer.env_states)
            bounced = any(st.pinned for st in peer.env_states)
            assert staged == prefetch, "prefetch staging used: %s" % staged
            assert bounced == pinned, "pinned bounce buffers used: %s" % bounced
        finally:
            P.close_peer(peer)
            del broker
        for check in ROW_CHECKS:
            check(batches, cfg)
        check_unroll_overlap(batches, cfg)


def _fixed_actor_input(B, device):
    g = torch.Generator().manual_seed(1234)
    return {
        "env": {
            "state": torch.randint(0, 256, (B, 4, 84, 84), dtype=torch.uint8, generator=g).to(device),
            "reward": torch.tensor([0.0, 1.0, -1.0, 0.5][:B]).to(device),
            "done": torch.zeros(B, dtype=torch.bool, device=device),
            "prev_action": (torch.arange(B) % 6).to(device),
        },
        "core": (),
    }


def _keep(res):
    return {k: res["out"][k].detach().clone() for k in ("policy_logits", "baseline")}


def _fresh_outputs(peer, inp):
    """A fresh AtariNet built from the CURRENT master weights the way the
    peer builds its forward model (same casts, same flat-buffer layout),
    run through ImpalaPeer._actor_fn: new modules, so new packed caches."""
    import copy

    from moolib_amd.models.atari import AtariNet

    cfg = peer.cfg
    master = AtariNet(num_actions=cfg.num_actions, use_lstm=cfg.use_lstm)
    master.load_state_dict(
        {k: v.detach().clone() for k, v in peer.model.state_dict().items()}
    )
    master.to(cfg.device)
    if cfg.channels_last:
        master.to(memory_format=torch.channels_last)
    fwd = master
    if peer.bf16_shadow:
        fwd = copy.deepcopy(master).to(torch.bfloat16)
        if cfg.channels_last:
            fwd.to(memory_format=torch.channels_last)
        flat = flatten_master_shadow(
            [p for p in master.parameters() if p.requires_grad],
            [p for p in fwd.parameters() if p.requires_grad],
        )
        for pm, pf in zip(master.parameters(), fwd.parameters()):
            assert torch.equal(pf.detach(), pm.detach().to(torch.bfloat16))
        del flat
    fwd.eval()
    shim = types.SimpleNamespace(fwd_model=fwd, autocast=peer.autocast, _actor_rng=None)
    return _keep(ImpalaPeer._actor_fn(shim, inp))


def _max_diff(a, b):
    return max((a[k].float() - b[k].float()).abs().max().item() for k in a)


@gpu
@requires_gpu
class TestWeightPropagation:
    """Whatever changes the master weights, the next actor forward (graph
    replay and eager) computes what a fresh model of those weights does."""

    @pytest.mark.timeout(180)
    @pytest.mark.parametrize("bf16_weights", [True, False], ids=["bf16w", "fp32w"])
    def test_actor_sees_current_weights(self, bf16_weights):
        from moolib_amd.envs import SyntheticAtariEnv

        broker, addr = P.make_broker()
        cfg = P.probe_config(
            addr, device="cuda:0", lr_schedule=False, bf16_weights=bf16_weights,
            seed=11, learning_rate=3e-3,
        )
        torch.manual_seed(11)
        peer = ImpalaPeer(cfg, lambda: SyntheticAtariEnv(num_actions=6), broker=broker)
        try:
            self._run(peer, bf16_weights)
        finally:
            P.close_peer(peer)
            del broker

    def _run(self, peer, bf16_weights):
        cfg = peer.cfg
        assert peer.bf16_shadow == bf16_weights and peer._graph_opt
        assert isinstance(peer._actor_call, GraphedCall)
        assert peer._actor_call.graph is not None, "actor graph not captured by prewarm"
        inp = _fixed_actor_input(cfg.actor_batch_size, cfg.device)
        peer.fwd_model.eval()

        # The yardstick: two fresh models of the same weights. Bit-equal
        # means exact comparison below; otherwise twice their difference.
        f1, f2 = _fresh_outputs(peer, inp), _fresh_outputs(peer, inp)
        noise = _max_diff(f1, f2)
        tol = 2.0 * noise
        print("ROLLOUT_FIGURE fresh_vs_fresh_max_abs_diff=%r bf16_weights=%s" % (noise, bf16_weights))

        def agree(got, want, what):
            if tol == 0.0:
                for k in want:
                    assert torch.equal(got[k], want[k]), "%s: %s differs by %r" % (
                        what, k, (got[k].float() - want[k].float()).abs().max().item())
            else:
                assert _max_diff(got, want) <= tol, (what, _max_diff(got, want), tol)

        def check(what, before):
            fresh = _fresh_outputs(peer, inp)
            # staleness would show: the new weights compute something else
            assert not torch.equal(fresh["policy_logits"], before["policy_logits"]), (
                "%s: changed weights give the old logits; the test cannot see staleness" % what)
            assert _max_diff(fresh, before) > tol
            agree(_keep(peer._actor_call(inp)), fresh, what + ", graph replay")
            agree(_keep(peer._actor_fn(inp)), fresh, what + ", eager")
            peer.fwd_model.eval()
            return fresh

        def drive(version):
            import time

            t0 = time.time()
            while peer.model_version < version and time.time() - t0 < 90:
                peer.step_once()
            assert peer.model_version == version
            peer.fwd_model.eval()

        agree(_keep(peer._actor_call(inp)), f1, "at construction, graph replay")
        agree(_keep(peer._actor_fn(inp)), f1, "at construction, eager")

        # (a) one eager optimizer step (the graph's warm-up phase)
        drive(1)
        assert peer._opt_call.graph is None and peer._opt_call.calls == 1
        fa = check("after an eager optimizer step", f1)

        # (b) optimizer steps past the warm-up: capture, then replays
        drive(peer._opt_call.warmup + 3)
        assert peer._opt_call.graph is not None and not peer._opt_call.failed
        fb = check("after graphed optimizer steps", fa)

        # (c) state sync: the accumulator writes the leader's parameters
        # into the master tensors in place, then step_once adopts the state
        g = torch.Generator(device=cfg.device).manual_seed(5)
        with torch.no_grad():
            for p in peer.model.parameters():
                p.copy_(p + 0.05 * torch.randn(p.shape, generator=g, device=p.device))
        peer._adopt_state(peer.save_state())
        check("after a state sync", fb)
        assert peer._actor_call.graph is not None and not peer._actor_call.failed


@gpu
@requires_gpu
class TestGraphedCallGpu:
    """The replay contract of GraphedCall on the device."""

    @staticmethod
    def _fn(i):
        return {"y": i["x"] * 2 + i["p"].float(), "z": (i["p"] + 1,)}

    def test_replays_track_inputs_and_match_eager(self):
        g = GraphedCall(self._fn, warmup=2, name="t_track")
        p = torch.zeros(5, dtype=torch.int64, device="cuda")  # persistent, like prev_action
        ptrs = []
        for n in range(7):
            x = torch.arange(5, device="cuda", dtype=torch.float32) + 10 * n  # new tensor
            p.copy_(torch.arange(5, device="cuda") * (n + 1))  # mutated in place
            out = g({"x": x, "p": p})
            want = self._fn({"x": x.clone(), "p": p.clone()})
            assert torch.equal(out["y"], want["y"]), n
            assert torch.equal(out["z"][0], want["z"][0]), n
            if g.graph is not None:
                ptrs.append((out["y"].data_ptr(), out["z"][0].data_ptr()))
        assert g.graph is not None and not g.failed
        # documented contract: the output nest is the same storage on every replay
        assert len(ptrs) == 5 and len(set(ptrs)) == 1, ptrs
        assert out["y"] is g.static_out["y"]

    def test_host_inputs_stay_eager(self):
        """Ops on host tensors are not recorded by a capture, so a "replay"
        would return the capture-time outputs for ever: with a device
        present, host inputs must fall back to eager and keep tracking."""
        calls = []

        def fn(i):
            calls.append(1)
            return {"y": i["x"] + 1}

        g = GraphedCall(fn, warmup=2, name="t_host")
        for n in range(6):
            out = g({"x": torch.full((3,), float(n))})
            assert torch.equal(out["y"], torch.full((3,), n + 1.0)), n
        assert len(calls) == 6 and g.failed and g.graph is None

    def test_generator_advances_and_is_reproducible(self):
        probs = torch.full((64, 16), 1.0 / 16, device="cuda")

        def sequence(seed):
            gen = torch.Generator(device="cuda")
            gen.manual_seed(seed)
            g = GraphedCall(
                lambda i: {"a": torch.multinomial(i["p"], 1, generator=gen)},
                warmup=2, name="t_rng", generators=[gen],
            )
            outs = [g({"p": probs})["a"].clone() for _ in range(6)]
            assert g.graph is not None and not g.failed
            return outs

        s1 = sequence(7)
        # calls 2.. are replays of the captured multinomial: each draws anew
        for a, b in zip(s1[2:-1], s1[3:]):
            assert not torch.equal(a, b)
        s2 = sequence(7)
        for n, (a, b) in enumerate(zip(s1, s2)):
            assert torch.equal(a, b), n
        s3 = sequence(8)
        assert not torch.equal(s1[-1], s3[-1])
