"""Actor priorities (ops.r2d2.actor_priorities) and moolib_amd.r2d2.SequenceBuilder.

docs/KERNEL_TESTS.md ("Actor priorities") has the definitions, the arguments
for the bounds and the recorded figures.

* The float64 reference `actor_priority_refs.actor_priority_ref` is explicit
  loops over k, t, i in numpy.
* Integer-exact cases (rescale off, small-integer inputs, discount 0.5): every
  output is exactly representable, so the fp32 eager path, the existing
  r2d2_loss on the lifted inputs and the kernel must be `torch.equal` to the
  reference.
* Float cases: the kernel's error against float64 is bounded by
  4 * max(e_ref, 2^-24 * scale), where e_ref is the error of the eager fp32 CPU
  path on the same inputs (computed here, never taken from the kernel), and
  every element stays within 1e-4 + 1e-5 |ref|.
* On the same inputs the kernel's TD errors are bit-identical to the loss
  kernel's (same device functions, same order); the priorities agree to one
  fp32 rounding.
* The builder is checked on leaves that encode (step, environment).
"""
import functools
import json

import numpy as np
import pytest
import torch

import actor_priority_refs as R
from moolib_amd.ops import r2d2 as ops

gpu = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

EPS = 1e-3
MAX_T = ops.KERNEL_MAX_T

# (T, K, n_step, burn_in): nothing valid; the smallest case with a valid step;
# n beyond the sequence; 4 and 8 valid steps; burn-in; 65 workgroups;
# burn_in = T-1 and burn_in > T (all zero); the limit on T. The number of
# valid steps is 0 or a power of two.
SHAPES = [
    (1, 1, 1, 0), (2, 1, 1, 0), (2, 3, 5, 0), (5, 3, 3, 0), (9, 5, 5, 0), (9, 5, 5, 4),
    (6, 65, 3, 1), (3, 2, 1, 2), (3, 2, 1, 7), (MAX_T, 2, 4, 127),
]
Q_SCALES = [1.0, 30.0]
INT_DISCOUNT = 0.5
FLOAT_DISCOUNT = 0.99
FLOAT_ETA = 0.9
LIFT_ACTIONS = 6


def _figure(**kw):
    """One machine-readable line per measured figure (shown with pytest -s)."""
    print("KERNEL_EDGES_FIGURE " + json.dumps(kw))


def _seed(shape):
    T, K, n, burn_in = shape
    return 1000 * T + 100 * K + 10 * n + burn_in


def tensors(case, device="cpu"):
    """q_taken, q_max, reward, done (bool) as torch tensors."""
    return tuple(torch.from_numpy(np.ascontiguousarray(case[k])).to(device)
                 for k in ("q_taken", "q_max", "reward", "done"))


@functools.lru_cache(maxsize=None)
def int_case(shape):
    return R.int_case(_seed(shape), shape[0], shape[1])


@functools.lru_cache(maxsize=None)
def int_ref(shape, eta):
    p, td = R.actor_priority_ref(int_case(shape), shape[2], INT_DISCOUNT, 0.0, False, eta, shape[3])
    return torch.from_numpy(p), torch.from_numpy(td)


def int_kwargs(shape, eta):
    return dict(n_step=shape[2], discount=INT_DISCOUNT, eps=0.0, rescale=False, eta=eta,
                burn_in=shape[3])


@functools.lru_cache(maxsize=None)
def float_case(shape, q_scale):
    return R.float_case(_seed(shape) + int(q_scale), shape[0], shape[1], q_scale)


@functools.lru_cache(maxsize=None)
def float_ref(shape, q_scale):
    p, td = R.actor_priority_ref(float_case(shape, q_scale), shape[2], FLOAT_DISCOUNT, EPS, True,
                                 FLOAT_ETA, shape[3])
    return {"priority": torch.from_numpy(p), "td": torch.from_numpy(td)}


def float_kwargs(shape):
    return dict(n_step=shape[2], discount=FLOAT_DISCOUNT, eps=EPS, rescale=True, eta=FLOAT_ETA,
                burn_in=shape[3])


@functools.lru_cache(maxsize=None)
def float_eager(shape, q_scale):
    """The fp32 eager path on the CPU."""
    out = ops.actor_priorities(*tensors(float_case(shape, q_scale)), **float_kwargs(shape))
    return {"priority": out.priorities, "td": out.td_errors}


def older_tolerance(ref):
    return 1e-4 + 1e-5 * ref.abs()


def kernel_bound(e_ref, ref):
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    return 4.0 * max(e_ref, 2.0 ** -24 * scale)


def within(got, ref, bound):
    """max|got - ref| <= bound and every element within the older tolerance;
    returns the error."""
    err = (got.double().cpu() - ref).abs()
    assert bool((err <= older_tolerance(ref)).all()), float(err.max())
    worst = float(err.max()) if err.numel() else 0.0
    assert worst <= bound, (worst, bound)
    return worst


def check_float(got_priority, got_td, shape, q_scale, tag):
    ref, eager = float_ref(shape, q_scale), float_eager(shape, q_scale)
    for name, got in (("priority", got_priority), ("td", got_td)):
        e_ref = float((eager[name].double() - ref[name]).abs().max())
        bound = kernel_bound(e_ref, ref[name])
        err = float((got.double().cpu() - ref[name]).abs().max())
        _figure(test=tag, case="%d %d %d %d %g" % (shape + (q_scale,)), tensor=name,
                e_ref=e_ref, err=err, bound=bound)
        within(got, ref[name], bound)


def shifted_loss_inputs(reward, done, discount, burn_in):
    """What R2D2Learner.learn feeds r2d2_loss: rewards and discounts that
    FOLLOW the action, the burn-in mask, unit weights."""
    T, K = reward.shape
    last = torch.zeros(1, K, device=reward.device)
    rewards = torch.cat([reward[1:], last], dim=0)
    discounts = torch.cat([discount * (~done[1:]).float(), last], dim=0)
    mask = torch.ones(T, K, device=reward.device)
    mask[:burn_in] = 0.0
    return rewards, discounts, mask, torch.ones(K, device=reward.device)


def lift(case, A=LIFT_ACTIONS):
    """q [T, K, A] whose taken entry is q_taken and whose unique maximum is
    q_max, and the actions; every other entry lies below both."""
    rng = np.random.RandomState(17)
    q_taken, q_max = case["q_taken"], case["q_max"]
    T, K = q_taken.shape
    greedy = rng.randint(0, A, size=(T, K))
    actions = (greedy + rng.randint(1, A, size=(T, K))) % A
    actions = np.where(q_taken == q_max, greedy, actions)
    q = (np.minimum(q_taken, q_max)[..., None] - 1.0 - rng.rand(T, K, A)).astype(np.float32)
    np.put_along_axis(q, actions[..., None], q_taken[..., None], axis=-1)
    np.put_along_axis(q, greedy[..., None], q_max[..., None], axis=-1)
    return torch.from_numpy(q), torch.from_numpy(actions)


# =============================================================== CPU: the op


class TestIntegerPremise:
    @pytest.mark.parametrize("shape", SHAPES)
    def test_reference_values_are_exact_in_fp32(self, shape):
        case = int_case(shape)
        assert shape[2] <= 5 and bool((case["q_max"] >= case["q_taken"]).all())
        valid = max(0, shape[0] - 1 - shape[3])
        assert valid == 0 or valid & (valid - 1) == 0
        for eta in (0.0, 1.0):
            p, td = int_ref(shape, eta)
            scaled = td * 2.0 ** 5
            assert torch.equal(scaled, scaled.round()) and float(scaled.abs().max()) < 2 ** 24
            assert float(td.abs().sum(0).max()) * 2 ** 5 < 2 ** 24
            assert torch.equal(p.float().double(), p)
        if valid == 0:
            assert not bool(td.any()) and not bool(p.any())

    @pytest.mark.parametrize("eta", [0.0, 1.0])
    @pytest.mark.parametrize("shape", SHAPES)
    def test_eager_fp32_equals_reference(self, shape, eta):
        p, td = int_ref(shape, eta)
        out = ops.actor_priorities(*tensors(int_case(shape)), **int_kwargs(shape, eta))
        assert out.td_errors.dtype == torch.float32 and out.td_errors.shape == shape[:2]
        assert out.priorities.shape == (shape[1],)
        assert torch.equal(out.td_errors.double(), td)
        assert torch.equal(out.priorities.double(), p)

    @pytest.mark.parametrize("eta", [0.0, 1.0])
    @pytest.mark.parametrize("shape", SHAPES)
    def test_equals_r2d2_loss_of_the_same_network(self, shape, eta):
        """The op is r2d2_loss with q_target = q on the learner's shifted
        rewards and discounts."""
        case = int_case(shape)
        p, td = int_ref(shape, eta)
        q = torch.from_numpy(case["q"])
        _, _, reward, done = tensors(case)
        rewards, discounts, mask, w = shifted_loss_inputs(reward, done, INT_DISCOUNT, shape[3])
        out = ops.r2d2_loss(q, q, torch.from_numpy(case["actions"]), rewards, discounts, mask, w,
                            n_step=shape[2], eps=0.0, rescale=False, eta=eta)
        assert torch.equal(out.td_errors.double(), td)
        assert torch.equal(out.priorities.double(), p)


class TestEagerCPU:
    @pytest.mark.parametrize("q_scale", Q_SCALES)
    @pytest.mark.parametrize("shape", SHAPES)
    def test_float_case_against_fp64(self, shape, q_scale):
        ref, got = float_ref(shape, q_scale), float_eager(shape, q_scale)
        for name in ("priority", "td"):
            err = (got[name].double() - ref[name]).abs()
            assert bool((err <= older_tolerance(ref[name])).all()), (name, float(err.max()))

    def test_uint8_done_noncontiguous_and_out(self):
        shape = (9, 5, 5, 4)
        q_taken, q_max, reward, done = tensors(float_case(shape, 1.0))
        want = float_eager(shape, 1.0)
        flip = lambda t: t.transpose(0, 1).contiguous().transpose(0, 1)
        assert not flip(q_taken).is_contiguous()
        out = (torch.full((5,), float("nan")), torch.full((9, 5), float("nan")))
        got = ops.actor_priorities(flip(q_taken), flip(q_max), flip(reward),
                                   flip(done.to(torch.uint8)), out=out, **float_kwargs(shape))
        assert got.priorities is out[0] and got.td_errors is out[1]
        assert torch.equal(got.priorities, want["priority"])
        assert torch.equal(got.td_errors, want["td"])

    def test_rewards_are_not_clipped_and_follow_the_action(self):
        # T = 2: delta_0 = reward[1] + g * q_max[1] - q_taken[0]; reward[0] is unused
        q_taken = torch.tensor([[1.0, 1.0], [9.0, 9.0]])
        q_max = torch.tensor([[7.0, 7.0], [2.0, 2.0]])
        reward = torch.tensor([[100.0, 100.0], [50.0, -50.0]])
        done = torch.tensor([[True, True], [False, True]])
        out = ops.actor_priorities(q_taken, q_max, reward, done, n_step=3, discount=0.5,
                                   rescale=False, eta=1.0)
        assert out.td_errors.tolist() == [[50.0, -51.0], [0.0, 0.0]]
        assert out.priorities.tolist() == [50.0, 51.0]

    def test_rejects_bad_arguments(self):
        args = tensors(int_case((5, 3, 3, 0)))
        for kw in ({"n_step": 0}, {"eps": -1e-3}, {"eta": 1.5}, {"eta": -0.1}, {"burn_in": -1}):
            with pytest.raises(ValueError, match="actor_priorities"):
                ops.actor_priorities(*args, **kw)
        with pytest.raises(ValueError, match="actor_priorities"):
            ops.actor_priorities(args[0], args[1][:4], args[2], args[3])
        with pytest.raises(ValueError, match="actor_priorities"):
            ops.actor_priorities(args[0][0], args[1][0], args[2][0], args[3][0])


# ========================================================== CPU: the builder

BUILDER_CONFIGS = [(4, 4, 12), (4, 2, 12), (5, 2, 13), (3, 1, 7)]
NUM_ENVS = 3
PRIORITY_KW = dict(n_step=2, discount=0.9, eps=1e-3, eta=0.7, burn_in=1)


def coded_step(s, K, device):
    """Leaves that encode (step, env); reward and done feed the priority."""
    k = torch.arange(K)
    g = torch.Generator().manual_seed(50 + s)
    step = {
        "code": 100.0 * s + k.float(),
        "frame": (s * 16 + k.view(K, 1, 1) * 4 + torch.arange(4).view(1, 2, 2)).to(torch.uint8),
        "reward": torch.randn(K, generator=g),
        "done": torch.rand(K, generator=g) < 0.2,
    }
    q = torch.randn(2, K, generator=g)
    q_taken, q_max = q.min(dim=0).values, q.max(dim=0).values
    return {n: t.to(device) for n, t in step.items()}, q_taken.to(device), q_max.to(device)


def run_builder(unroll, period, steps, device, with_q=True, K=NUM_ENVS):
    """Feeds `steps` coded steps; the caller's core state is ONE pair of
    tensors overwritten in place, like the outputs of a captured graph.
    Returns {step index: emission} and snapshots taken at emission time."""
    from moolib_amd.r2d2 import SequenceBuilder

    b = SequenceBuilder(unroll, period, **PRIORITY_KW)
    h = torch.zeros(1, K, 2, device=device)
    c = torch.zeros(1, K, 2, device=device)
    emitted, snapshots = {}, {}
    for s in range(steps):
        h.fill_(float(s))
        c.fill_(-float(s))
        step, q_taken, q_max = coded_step(s, K, device)
        out = b.append(step, (h, c), q_taken, q_max) if with_q else b.append(step, (h, c))
        if out is not None:
            emitted[s] = out
            snapshots[s] = ({n: t.clone() for n, t in out[0].items()},
                            None if out[1] is None else out[1].clone())
    return emitted, snapshots


def check_builder(unroll, period, steps, device):
    K = NUM_ENVS
    emitted, snapshots = run_builder(unroll, period, steps, device)
    want_steps = [s for s in range(steps)
                  if s + 1 >= unroll and (s + 1 - unroll) % period == 0]
    assert sorted(emitted) == want_steps and len(want_steps) >= 2
    for j, s in enumerate(want_steps):
        items, priorities = emitted[s]
        first = j * period
        assert first + unroll == s + 1
        rows = [coded_step(first + i, K, "cpu") for i in range(unroll)]
        assert set(items) == {"code", "frame", "reward", "done", "core_h", "core_c"}
        for name in ("code", "frame", "reward", "done"):
            want = torch.stack([r[0][name] for r in rows])
            assert items[name].dtype == want.dtype and items[name].shape == want.shape
            assert torch.equal(items[name].cpu(), want), (name, j)
        assert items["frame"].shape == (unroll, K, 2, 2)
        # the state passed WITH the window's first step, although the caller
        # has overwritten that tensor since
        assert torch.equal(items["core_h"].cpu(), torch.full((1, K, 2), float(first)))
        assert torch.equal(items["core_c"].cpu(), torch.full((1, K, 2), -float(first)))
        want = ops.actor_priorities(
            torch.stack([r[1] for r in rows]).to(device), torch.stack([r[2] for r in rows]).to(device),
            items["reward"], items["done"], **PRIORITY_KW).priorities
        assert priorities.shape == (K,) and torch.equal(priorities, want)
        # later appends left this emission alone
        for name, t in snapshots[s][0].items():
            assert torch.equal(items[name], t), (name, j)
        assert torch.equal(priorities, snapshots[s][1])


class TestBuilderCPU:
    @pytest.mark.parametrize("unroll,period,steps", BUILDER_CONFIGS)
    def test_windows_states_and_priorities(self, unroll, period, steps):
        check_builder(unroll, period, steps, "cpu")

    def test_no_q_values_no_priorities_and_no_core(self):
        from moolib_amd.r2d2 import SequenceBuilder

        emitted, _ = run_builder(4, 2, 8, "cpu", with_q=False)
        assert sorted(emitted) == [3, 5, 7]
        assert all(p is None for _, p in emitted.values())
        b = SequenceBuilder(2)  # period None: disjoint windows; no core
        assert b.period == 2
        outs = [b.append(coded_step(s, 2, "cpu")[0], ()) for s in range(4)]
        assert outs[0] is None and outs[2] is None
        for j, out in ((0, outs[1]), (1, outs[3])):
            items, priorities = out
            assert priorities is None and set(items) == {"code", "frame", "reward", "done"}
            assert items["code"][:, 0].tolist() == [200.0 * j, 200.0 * j + 100.0]

    def test_argument_errors(self):
        from moolib_amd.r2d2 import SequenceBuilder

        for period in (0, 5, -1):
            with pytest.raises(ValueError, match="period"):
                SequenceBuilder(4, period)
        step, q_taken, q_max = coded_step(0, 3, "cpu")
        for missing in ("reward", "done"):
            bad = {k: v for k, v in step.items() if k != missing}
            with pytest.raises(ValueError, match=missing):
                SequenceBuilder(4, 2).append(bad, (), q_taken, q_max)
        b = SequenceBuilder(4, 2)
        assert b.append(step, (), q_taken, q_max) is None
        with pytest.raises(ValueError, match="environments"):
            b.append(*((coded_step(1, 4, "cpu")[0], ()) + coded_step(1, 4, "cpu")[1:]))
        with pytest.raises(ValueError, match="Q-values"):
            b.append(coded_step(1, 3, "cpu")[0], ())
        with pytest.raises(ValueError, match="together"):
            b.append(step, (), q_taken, None)

    def test_learner_entry_point(self):
        from moolib_amd.r2d2 import R2D2Config, R2D2Learner, SequenceBuilder

        cfg = R2D2Config(n_step=3, discount=0.9, eps=1e-2, eta=0.5, burn_in=2)
        b = R2D2Learner(CoreNet(), cfg, "cpu").sequence_builder(8, 4)
        assert isinstance(b, SequenceBuilder) and (b.unroll, b.period) == (8, 4)
        assert b.priority_args == dict(n_step=3, discount=0.9, eps=1e-2, eta=0.5, burn_in=2)
        assert R2D2Learner(CoreNet(), cfg, "cpu").sequence_builder(8).period == 8


# ================================================================ end to end


class CoreNet(torch.nn.Module):
    """AtariNet's forward contract on a vector observation, with an LSTM core
    that is reset where done."""

    def __init__(self, num_actions=5):
        super().__init__()
        self.body = torch.nn.Linear(7, 8)
        self.core = torch.nn.LSTM(8, 8)
        self.policy = torch.nn.Linear(8, num_actions)
        self.baseline = torch.nn.Linear(8, 1)

    def initial_state(self, batch_size=1):
        return tuple(torch.zeros(1, batch_size, 8) for _ in range(2))

    def forward(self, inputs, core_state):
        T, B = inputs["reward"].shape
        x = torch.relu(self.body(inputs["state"].float()))
        outs = []
        for t in range(T):
            nd = (~inputs["done"][t]).float().view(1, B, 1)
            core_state = tuple(nd * s for s in core_state)
            o, core_state = self.core(x[t:t + 1], core_state)
            outs.append(o)
        y = torch.cat(outs)
        out = {"policy_logits": self.policy(y).float(),
               "baseline": self.baseline(y).float().view(T, B)}
        return out, core_state


def check_end_to_end(device, fused_act):
    from moolib_amd.r2d2 import R2D2Config, R2D2Learner
    from moolib_amd.replay import SumTreeReplayBuffer

    unroll, period, K, alpha = 6, 3, 4, 0.9
    torch.manual_seed(1)
    cfg = R2D2Config(n_step=3, burn_in=1, epsilon=0.3, lr=1e-2, fused_act=fused_act, seed=5)
    learner = R2D2Learner(CoreNet(), cfg, device, autocast=False)
    builder = learner.sequence_builder(unroll, period)
    buf = SumTreeReplayBuffer(16, device=device, alpha=alpha, beta=0.6)
    core = tuple(s.to(device) for s in learner.online.initial_state(K))
    prev_action = torch.zeros(K, dtype=torch.int64, device=device)
    g = torch.Generator().manual_seed(8)
    emitted = []
    for s in range(unroll + period):
        step = {
            "state": torch.randn(K, 7, generator=g).to(device),
            "reward": torch.randn(K, generator=g).to(device),
            "done": (torch.rand(K, generator=g) < 0.15).to(device),
            "prev_action": prev_action,
        }
        inputs = {k: v.unsqueeze(0) for k, v in step.items()}
        action, new_core, (q_taken, q_max) = learner.act(inputs, core, return_q=True)
        step["action"] = action.squeeze(0)
        out = builder.append(step, core, q_taken, q_max)
        core, prev_action = new_core, step["action"]
        if out is not None:
            emitted.append(out)
    assert len(emitted) == 2
    for items, priorities in emitted:
        assert priorities.device.type == torch.device(device).type
        assert bool(torch.isfinite(priorities).all()) and float(priorities.max()) > 0
        buf.add_batch(items, priorities, batch_dim=1)
    assert len(buf) == 2 * K
    p = torch.cat([p for _, p in emitted]).double().cpu()
    want = p.clamp_min(1e-6) ** alpha
    err = (buf.priorities[:2 * K].double().cpu() - want).abs()
    # one fp32 rounding of the leaf, the bound of the sum-tree tests
    assert bool((err <= 2.0 ** -23 * want).all()), float((err / want).max())
    assert not bool(buf.priorities[2 * K:].any())

    items, idx, w = buf.sample(3, time_major=True)
    batch = {k: items[k] for k in ("state", "reward", "done", "prev_action", "action")}
    batch["core_state"] = (items["core_h"], items["core_c"])
    assert batch["reward"].shape == (unroll, 3) and batch["core_state"][0].shape == (1, 3, 8)
    before = [q.detach().clone() for q in learner.online.parameters()]
    metrics, new_p = learner.learn(batch, w)
    assert new_p.shape == (3,) and bool(torch.isfinite(new_p).all())
    assert bool(torch.isfinite(metrics["loss"]))
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, learner.online.parameters()))
    buf.update_priorities(idx, new_p)


class TestEndToEndCPU:
    @pytest.mark.parametrize("fused_act", [False, True])
    def test_act_builder_replay_learn(self, fused_act):
        check_end_to_end("cpu", fused_act)

    @staticmethod
    def _example():
        import importlib.util
        import os

        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                            "examples", "r2d2.py")
        spec = importlib.util.spec_from_file_location("r2d2_example", path)
        example = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(example)
        return example

    @pytest.mark.parametrize("sumtree", [True, False])
    def test_example_with_overlap_and_actor_priorities(self, sumtree):
        import math

        m = self._example().run(device="cpu", capacity=64, unroll=4, burn_in=1, batch_size=4,
                                num_envs=4, seconds=2.0, sumtree=sumtree, period=2,
                                actor_priorities=True)
        assert m["period"] == 2 and m["actor_priorities"] is True
        assert m["buffer_seqs"] >= 8 and m["buffer_seqs"] % 4 == 0
        # one sequence of 4 environments every 2 steps once the first is full
        steps = m["frames_acted"] // 4
        assert min(64, 4 * ((steps - 4) // 2 + 1)) == m["buffer_seqs"]
        assert math.isfinite(m["initial_priority_mean"]) and m["initial_priority_mean"] > 0
        assert m["learn_steps"] > 0 and math.isfinite(m["loss"])

    def test_example_defaults_never_build_sequences(self, monkeypatch):
        """run() with default arguments takes the Batcher path: it never
        constructs a SequenceBuilder and never asks the act head for Q-values."""
        import moolib_amd.r2d2 as mod

        example = self._example()

        class Forbidden:
            def __init__(self, *a, **kw):
                raise AssertionError("SequenceBuilder constructed on the default path")

        monkeypatch.setattr(mod, "SequenceBuilder", Forbidden)
        real_act = mod.R2D2Learner.act

        def act(self, *a, **kw):
            assert not kw.get("return_q"), "return_q on the default path"
            return real_act(self, *a, **kw)

        monkeypatch.setattr(mod.R2D2Learner, "act", act)
        m = example.run(device="cpu", capacity=8, unroll=2, burn_in=0, batch_size=2, num_envs=2,
                        seconds=0.5, min_replay=10 ** 9)
        assert "initial_priority_mean" not in m and m["frames_acted"] > 0
        # the patch is what the entry point on the learner would construct
        with pytest.raises(AssertionError, match="default path"):
            mod.R2D2Learner(CoreNet(), None, "cpu").sequence_builder(4)


# =============================================================== GPU tests


def kernel_call(case, kwargs, done_dtype=torch.bool):
    """The op on the GPU, writing into NaN-filled buffers."""
    q_taken, q_max, reward, done = tensors(case, "cuda")
    T, K = q_taken.shape
    out = (torch.full((K,), float("nan"), device="cuda"),
           torch.full((T, K), float("nan"), device="cuda"))
    got = ops.actor_priorities(q_taken, q_max, reward, done.to(done_dtype), out=out, **kwargs)
    assert got.priorities.data_ptr() == out[0].data_ptr()
    assert got.td_errors.data_ptr() == out[1].data_ptr()
    return got


@gpu
@requires_gpu
class TestKernel:
    @pytest.fixture(autouse=True)
    def _kernel_path(self, monkeypatch):
        monkeypatch.delenv("MOOLIB_AMD_NO_R2D2_KERNEL", raising=False)
        assert ops._kernels() is not None

    @pytest.mark.parametrize("eta", [0.0, 1.0])
    @pytest.mark.parametrize("shape", SHAPES)
    def test_integer_exact(self, shape, eta):
        p, td = int_ref(shape, eta)
        got = kernel_call(int_case(shape), int_kwargs(shape, eta))
        assert torch.equal(got.td_errors.cpu().double(), td)
        assert torch.equal(got.priorities.cpu().double(), p)
        if shape[0] - 1 <= shape[3]:
            assert not bool(got.td_errors.any()) and not bool(got.priorities.any())

    @pytest.mark.parametrize("q_scale", Q_SCALES)
    @pytest.mark.parametrize("shape", SHAPES)
    def test_float_case(self, shape, q_scale):
        got = kernel_call(float_case(shape, q_scale), float_kwargs(shape))
        check_float(got.priorities, got.td_errors, shape, q_scale, "actor_priority")

    @pytest.mark.parametrize("q_scale", Q_SCALES)
    @pytest.mark.parametrize("shape", SHAPES)
    def test_agrees_with_the_loss_kernel(self, shape, q_scale):
        case = float_case(shape, q_scale)
        got = kernel_call(case, float_kwargs(shape))
        q, actions = lift(case)
        assert torch.equal(q.max(dim=-1).values, torch.from_numpy(case["q_max"]))
        _, _, reward, done = tensors(case, "cuda")
        rewards, discounts, mask, w = shifted_loss_inputs(reward, done, FLOAT_DISCOUNT, shape[3])
        q = q.cuda()
        loss = ops.r2d2_loss(q, q, actions.cuda(), rewards, discounts, mask, w,
                             n_step=shape[2], eps=EPS, rescale=True, eta=FLOAT_ETA)
        assert torch.equal(got.td_errors, loss.td_errors)
        ref = float_ref(shape, q_scale)["priority"]
        diff = (got.priorities.double() - loss.priorities.double()).abs().cpu()
        assert bool((diff <= 2.0 ** -23 * ref.abs()).all()), float(diff.max())

    def test_bit_reproducible(self):
        shape = (6, 65, 3, 1)
        a = kernel_call(float_case(shape, 30.0), float_kwargs(shape))
        b = ops.actor_priorities(*tensors(float_case(shape, 30.0), "cuda"), **float_kwargs(shape))
        assert torch.equal(a.td_errors, b.td_errors) and torch.equal(a.priorities, b.priorities)

    def test_bool_and_uint8_done_agree(self):
        shape = (9, 5, 5, 4)
        a = kernel_call(float_case(shape, 1.0), float_kwargs(shape))
        b = kernel_call(float_case(shape, 1.0), float_kwargs(shape), done_dtype=torch.uint8)
        assert torch.equal(a.td_errors, b.td_errors) and torch.equal(a.priorities, b.priorities)
        assert bool(torch.from_numpy(float_case(shape, 1.0)["done"])[1:].any())

    def test_noncontiguous_inputs(self):
        shape = (9, 5, 5, 4)
        want = kernel_call(float_case(shape, 1.0), float_kwargs(shape))
        flip = lambda t: t.transpose(0, 1).contiguous().transpose(0, 1)
        args = [flip(t) for t in tensors(float_case(shape, 1.0), "cuda")]
        assert not any(t.is_contiguous() for t in args)
        got = ops.actor_priorities(*args, **float_kwargs(shape))
        assert torch.equal(got.td_errors, want.td_errors)
        assert torch.equal(got.priorities, want.priorities)

    def test_host_checks(self):
        from moolib_amd import _kernels

        T, K = 4, 3
        good = dict(zip(("q_taken", "q_max", "reward", "done"),
                        tensors(float_case((T, K, 2, 0), 1.0), "cuda")))

        def call(n=2, discount=0.99, eps=EPS, eta=0.9, burn_in=0, **override):
            a = dict(good, **override)
            return _kernels.r2d2_actor_priority(a["q_taken"], a["q_max"], a["reward"], a["done"],
                                                n, discount, eps, True, eta, burn_in)

        call()
        call(burn_in=T - 1)
        call(burn_in=10 ** 6)
        flip = lambda t: t.transpose(0, 1).contiguous().transpose(0, 1)
        bad = [
            dict(q_taken=good["q_taken"].double()),
            dict(reward=good["reward"].half()),
            dict(done=good["done"].float()),
            dict(done=good["done"].long()),
            dict(q_max=good["q_max"].cpu()),
            dict(q_taken=good["q_taken"].cpu()),
            dict(done=good["done"].cpu()),
            dict(q_max=good["q_max"][:3].contiguous()),
            dict(reward=good["reward"][:, :2].contiguous()),
            dict(done=good["done"].view(-1)),
            dict(q_taken=flip(good["q_taken"])),
            dict(reward=flip(good["reward"])),
            dict(done=flip(good["done"])),
            dict(n=0),
            dict(eps=-1.0),
            dict(eta=1.5),
            dict(eta=-0.5),
            dict(burn_in=-1),
        ]
        for kw in bad:
            with pytest.raises(RuntimeError, match="r2d2_actor_priority"):
                call(**kw)
        long = tensors(R.float_case(2, MAX_T + 1, 1, 1.0), "cuda")
        with pytest.raises(RuntimeError, match="r2d2_actor_priority.*limit"):
            _kernels.r2d2_actor_priority(*long, 2, 0.99, EPS, True, 0.9, 0)
        with pytest.raises(RuntimeError, match="r2d2_actor_priority.*td_out"):
            _kernels.r2d2_actor_priority(*[good[k] for k in ("q_taken", "q_max", "reward", "done")],
                                         2, 0.99, EPS, True, 0.9, 0, None,
                                         torch.empty(T + 1, K, device="cuda"))

    def test_eager_path_on_the_gpu(self, monkeypatch):
        shape, q_scale = (6, 65, 3, 1), 30.0
        monkeypatch.setenv("MOOLIB_AMD_NO_R2D2_KERNEL", "1")
        assert ops._kernels() is None
        got = ops.actor_priorities(*tensors(float_case(shape, q_scale), "cuda"),
                                   **float_kwargs(shape))
        check_float(got.priorities, got.td_errors, shape, q_scale, "actor_priority_eager_gpu")

    def test_graph_replay_follows_new_inputs(self):
        shape = (9, 5, 5, 4)
        first, second = float_case(shape, 1.0), float_case(shape, 30.0)
        static = [t.clone() for t in tensors(first, "cuda")]
        out = (torch.full((5,), float("nan"), device="cuda"),
               torch.full((9, 5), float("nan"), device="cuda"))
        ops.actor_priorities(*static, out=out, **float_kwargs(shape))  # loads the code object
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ops.actor_priorities(*static, out=out, **float_kwargs(shape))
        for case in (second, first):
            for dst, src in zip(static, tensors(case, "cuda")):
                dst.copy_(src)
            out[0].fill_(float("nan"))
            out[1].fill_(float("nan"))
            g.replay()
            want = ops.actor_priorities(*tensors(case, "cuda"), **float_kwargs(shape))
            assert torch.equal(out[0], want.priorities) and torch.equal(out[1], want.td_errors)
        assert not torch.equal(*[ops.actor_priorities(*tensors(c, "cuda"),
                                                      **float_kwargs(shape)).priorities
                                 for c in (first, second)])


@gpu
@requires_gpu
class TestBuilderAndLearnerGPU:
    def test_builder_on_the_gpu(self):
        check_builder(5, 2, 13, "cuda")

    def test_act_builder_replay_learn_fused_act(self):
        check_end_to_end("cuda", fused_act=True)
