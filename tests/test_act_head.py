"""Fused actor head: Philox action sampling and the epsilon-greedy dueling head.

docs/KERNEL_TESTS.md ("Action head") has the premises and bounds.

* Philox4x32-10 is pinned by three known answers; `philox_uniforms` (int64
  tensor arithmetic) must equal the Python-integer reference of act_refs.
* The epsilon-greedy head is exact integers and single IEEE operations, so
  the eager path must equal the fp64/integer reference bit for bit, and the
  kernel must equal the eager path bit for bit.
* With logits in {0, -inf} every e_a is exactly 0 or 1 and the categorical
  draw is exact too. Elsewhere the kernel is held to the fp64 CDF on every
  row that is decidable under DELTA (derived at `categorical_delta`).
* A launch with `state` must equal the launch with `u = philox_uniforms(seed,
  step, N)` and leave `step + 1`, replays of a captured launch included.
"""
import functools

import numpy as np
import pytest
import torch

import act_refs as R
from moolib_amd.ops import act as ops

gpu = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

ACTIONS = [1, 2, 3, 18, 64]
ROWS = [1, 2, 63, 64, 65, 1023, 1024, 1025, 2049]
U_TOP = 1.0 - 2.0 ** -24  # the largest uniform

KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def categorical_delta(A):
    """Relative distance to a CDF boundary under which the fp32 kernel may
    decide a row differently from the fp64 reference.

    With x_a = l_a - m <= 0 and total >= 1 (the maximum contributes e^0), the
    kernel's terms are e_a (1 + th_a): expf is within 1 ulp (2^-23 relative),
    and the fp32 subtraction perturbs x_a by at most 2^-24 |x_a|, i.e. e_a by
    2^-24 |x_a| e^(x_a) <= 2^-24 / e. Over a row the terms' error is at most
    (1 + (A-1) / (2e)) 2^-23 total, and the A-1 ordered additions add at most
    (A-1) 2^-24 total, so a running sum is off by at most
        E = (1 + 0.19 (A-1) + 0.5 (A-1)) 2^-23 total.
    The target u0 * total carries the error of `total` (E again, u0 < 1) and
    one rounding (2^-24 total). A comparison can flip only within
        2E + 2^-24 total  <=  (1.38 A + 1.2) 2^-23 total,
    rounded up to (1.5 A + 2) 2^-23. (Second-order terms are below 2^-40.)
    """
    return (1.5 * A + 2.0) * 2.0 ** -23


# ------------------------------------------------------------------ inputs


@functools.lru_cache(maxsize=None)
def uniforms_for(N, seed, edges=True):
    """u [N, 2] on the 2^-24 grid, with the edges in the first rows."""
    g = torch.Generator().manual_seed(1000 + seed)
    u = torch.randint(0, 1 << 24, (N, 2), generator=g).float() * 2.0 ** -24
    if edges:
        first = torch.tensor([[0.0, 0.0], [U_TOP, U_TOP], [0.5, U_TOP], [U_TOP, 0.0],
                              [0.0, 1.0]])  # u1 = 1: the A - 1 clamp
        k = min(N, first.shape[0])
        u[:k] = first[:k]
    return u


@functools.lru_cache(maxsize=None)
def eps_greedy_case(N, A):
    """value, advantage (quantised so that ties on the maximum are common),
    epsilon (0, 1 and values between), u; with the reference's outputs."""
    g = torch.Generator().manual_seed(7 * N + A)
    value = torch.randn(N, generator=g)
    adv = torch.randn(N, A, generator=g)
    adv[::2] = torch.round(adv[::2] * 2) / 2  # ties
    if N > 2:
        adv[2] = 0.25  # a whole row tied
    eps = torch.rand(N, generator=g)
    eps[::3] = 0.0
    eps[1::3] = 1.0
    u = uniforms_for(N, A)
    ref = R.eps_greedy_ref(value.numpy(), adv.numpy(), eps.numpy(), u.numpy())
    return value, adv, eps, u, ref


@functools.lru_cache(maxsize=None)
def logits_case(N, A, scale):
    g = torch.Generator().manual_seed(31 * N + A + int(scale))
    logits = torch.randn(N, A, generator=g) * scale
    # no edge rows: u0 = U_TOP is within 2^-24 of the top boundary and u0 = 0
    # on the bottom one, never decidable; the exact {0, -inf} cases cover them
    u = uniforms_for(N, 100 + A, edges=False)
    return logits, u, R.categorical_ref(logits.numpy(), u[:, 0].numpy())


@functools.lru_cache(maxsize=None)
def masked_case(A):
    """Logits in {0, -inf}: every mask with a single live action, random
    masks, against every edge u0 and a sweep. For u0 < 1 the fp32 product
    u0 * total stays below total (total * 2^-24 is at least half an ulp of
    total, and the tie at a power of two lands on a representable number), so
    the target reaches `total`, where no running sum exceeds it, only for the
    explicit u0 = 1; that row takes the last live action."""
    g = torch.Generator().manual_seed(5 + A)
    masks = [torch.eye(A, dtype=torch.bool)]
    masks.append(torch.rand(64, A, generator=g) < 0.5)
    masks.append(torch.ones(1, A, dtype=torch.bool))
    mask = torch.cat(masks)
    mask[mask.sum(dim=1) == 0, A - 1] = True
    u0 = torch.cat([
        torch.tensor([0.0, U_TOP, 1.0, 0.5, 2.0 ** -24, 1.0 - 2.0 ** -23, 1.0 / 3, 2.0 / 3]),
        torch.arange(9) / 8.0 * U_TOP,
    ]).float()
    logits = torch.where(mask, 0.0, float("-inf")).float()
    logits = logits.repeat_interleave(u0.numel(), dim=0)
    u0 = u0.repeat(mask.shape[0])
    u = torch.stack([u0, torch.zeros_like(u0)], dim=1)
    ref = R.masked_categorical_ref(logits.numpy(), u0.numpy())
    return logits, u, torch.from_numpy(ref)


def assert_eps_greedy(got, ref):
    action, q_taken, q_max = (t.cpu() for t in got)
    assert action.dtype == torch.int64
    assert torch.equal(action, torch.from_numpy(ref[0]))
    # bit for bit: compare the words, so that -0.0 and 0.0 differ
    assert torch.equal(q_taken.view(torch.int32), torch.from_numpy(ref[1]).view(torch.int32))
    assert torch.equal(q_max.view(torch.int32), torch.from_numpy(ref[2]).view(torch.int32))


# ------------------------------------------------------------------ Philox


class TestPhilox:
    @pytest.mark.parametrize("counter,key,out", KNOWN_ANSWERS)
    def test_known_answers_reference(self, counter, key, out):
        assert R.philox4x32(counter, key) == out

    @pytest.mark.parametrize("counter,key,out", KNOWN_ANSWERS)
    def test_known_answers_op_words(self, counter, key, out):
        words = ops._philox4x32([torch.tensor([c], dtype=torch.int64) for c in counter], key)
        assert tuple(int(w) for w in words) == out

    def test_first_known_answer_through_uniforms(self):
        u = ops.philox_uniforms(0, 0, 1)
        assert u.dtype == torch.float32 and u.shape == (1, 2)
        assert float(u[0, 0]) * 2 ** 24 == 0x6627E8D5 >> 8
        assert float(u[0, 1]) * 2 ** 24 == 0xE169C58D >> 8

    @pytest.mark.parametrize("seed", [0, 12345, -1, (1 << 63) - 1, -(1 << 63)])
    @pytest.mark.parametrize("step", [0, 1, (1 << 32) - 1, 1 << 32, (1 << 40) + 7])
    def test_uniforms_equal_reference(self, seed, step):
        n = (1 << 20) + 1
        u = ops.philox_uniforms(seed, step, n)
        rows = [0, 1, 2, 1023, 1 << 20]
        assert torch.equal(u[rows], torch.from_numpy(R.uniforms(seed, step, rows)))
        assert float(u.max()) < 1.0 and float(u.min()) >= 0.0
        scaled = u.double() * 2 ** 24
        assert torch.equal(scaled, scaled.floor())

    def test_seed_minus_one_is_all_ones(self):
        assert R.counter_and_key(-1, 0, 0)[1] == (0xFFFFFFFF, 0xFFFFFFFF)
        assert torch.equal(ops.philox_uniforms(-1, 5, 4), ops.philox_uniforms((1 << 64) - 1, 5, 4))

    def test_step_carries_into_word_three(self):
        lo = R.counter_and_key(9, (1 << 32) - 1, 0)[0]
        hi = R.counter_and_key(9, 1 << 32, 0)[0]
        assert lo == (0, 0, 0xFFFFFFFF, 0) and hi == (0, 0, 0, 1)
        a = ops.philox_uniforms(9, (1 << 32) - 1, 8)
        b = ops.philox_uniforms(9, 1 << 32, 8)
        c = ops.philox_uniforms(9, 0, 8)
        assert not torch.equal(a, b) and not torch.equal(b, c)

    def test_new_state(self):
        s = ops.new_state(-1)
        assert s.dtype == torch.int64 and s.tolist() == [-1, 0]
        assert ops.new_state((1 << 64) - 1).tolist() == [-1, 0]
        assert ops.new_state(7).tolist() == [7, 0]


# -------------------------------------------------------------- CPU, eager


class TestEpsGreedyCPU:
    @pytest.mark.parametrize("A", ACTIONS)
    def test_eager_equals_reference(self, A):
        value, adv, eps, u, ref = eps_greedy_case(257, A)
        assert_eps_greedy(ops.epsilon_greedy_dueling(value, adv, eps, u=u), ref)

    @pytest.mark.parametrize("A", ACTIONS)
    def test_ties_epsilon_ends_and_clamp(self, A):
        N = 8
        value = torch.zeros(N)
        adv = torch.full((N, A), 0.5)  # all tied: the greedy action is 0
        u = torch.tensor([[0.0, U_TOP]]).repeat(N, 1)
        # epsilon 0 never explores, not even at u0 == 0
        a, qt, qm = ops.epsilon_greedy_dueling(value, adv, 0.0, u=u)
        assert torch.equal(a, torch.zeros(N, dtype=torch.int64)) and torch.equal(qt, qm)
        # epsilon 1 always explores, even at the largest u0; u1 at its
        # largest value lands on A - 1. (fp32 u1 * A stays below A for every
        # u1 < 1; the explicit u1 = 1 of the second half is what needs the
        # clamp.)
        u = torch.tensor([[U_TOP, U_TOP]]).repeat(N, 1)
        u[N // 2:, 1] = 1.0
        a, _, _ = ops.epsilon_greedy_dueling(value, adv, torch.ones(N), u=u)
        assert torch.equal(a, torch.full((N,), A - 1, dtype=torch.int64))
        ref = R.eps_greedy_ref(value.numpy(), adv.numpy(), np.ones(N, np.float32), u.numpy())
        assert_eps_greedy(ops.epsilon_greedy_dueling(value, adv, 1.0, u=u), ref)

    def test_lowest_index_wins_ties(self):
        adv = torch.tensor([[1.0, 3.0, 3.0, 2.0], [5.0, 5.0, 5.0, 5.0], [0.0, 1.0, 0.0, 1.0]])
        a, qt, qm = ops.epsilon_greedy_dueling(torch.zeros(3), adv, 0.0, u=torch.zeros(3, 2))
        assert a.tolist() == [1, 0, 1]
        assert torch.equal(qt, qm)

    def test_leading_dimensions_and_state(self):
        value, adv, eps, _, _ = eps_greedy_case(6, 3)
        state = ops.new_state(11)
        state[1] = 4
        got = ops.epsilon_greedy_dueling(value.view(2, 3), adv.view(2, 3, 3), eps.view(2, 3),
                                         state=state)
        assert all(t.shape == (2, 3) for t in got)
        assert state.tolist() == [11, 5]
        want = ops.epsilon_greedy_dueling(value, adv, eps, u=ops.philox_uniforms(11, 4, 6))
        for g, w in zip(got, want):
            assert torch.equal(g.reshape(-1), w)


class TestCategoricalCPU:
    @pytest.mark.parametrize("A", ACTIONS)
    def test_masked_logits_exact(self, A):
        logits, u, ref = masked_case(A)
        action = ops.sample_categorical(logits, u=u)
        assert action.dtype == torch.int64
        assert torch.equal(action, ref)
        assert bool((logits.gather(1, action.unsqueeze(1)) == 0).all()), "a masked action"

    def test_top_rounding_takes_the_last_live_action(self):
        # target == total = 3: no running sum exceeds it
        logits = torch.tensor([[0.0, float("-inf"), 0.0, 0.0, float("-inf")]])
        u = torch.tensor([[1.0, 0.0]])
        assert ops.sample_categorical(logits, u=u).tolist() == [3]
        # the largest uniform stays below: 3 (1 - 2^-24) rounds to 3 - 2^-22
        assert np.float32(U_TOP) * np.float32(3) < np.float32(3)
        u = torch.tensor([[U_TOP, 0.0]])
        assert ops.sample_categorical(logits, u=u).tolist() == [3]

    @pytest.mark.parametrize("scale", [1.0, 4.0, 16.0])
    def test_reference_leaves_no_row_undecidable(self, scale):
        """The premise of the GPU check, and the eager path held to it."""
        _, _, (_, margin, _) = logits_case(4096, 18, scale)
        assert int((margin <= categorical_delta(18)).sum()) == 0
        logits, u, (ref, _, _) = logits_case(4096, 18, scale)
        assert torch.equal(ops.sample_categorical(logits, u=u), torch.from_numpy(ref))

    @pytest.mark.parametrize("A", ACTIONS)
    def test_reference_premise_at_the_gpu_shapes(self, A):
        """At most 1% of the rows of every GPU case are undecidable, and the
        eager path meets the GPU check too."""
        for N in ROWS:
            for scale in (1.0, 16.0):
                logits, u, (ref, margin, nearest) = logits_case(N, A, scale)
                near = margin <= categorical_delta(A)
                assert near.sum() <= 0.01 * N
                got = ops.sample_categorical(logits, u=u).numpy()
                assert np.array_equal(got[~near], ref[~near])

    def test_chi_square(self):
        """16384 draws of one logit row at a fixed seed against its softmax:
        chi-square (17 degrees of freedom) below the 99.9% quantile 40.790."""
        N, A = 16384, 18
        row = torch.linspace(-1.5, 1.5, A)
        state = ops.new_state(20261021)
        action = ops.sample_categorical(row.expand(N, A), state=state)
        assert state.tolist() == [20261021, 1]
        p = torch.softmax(row.double(), dim=0)
        counts = torch.bincount(action, minlength=A).double()
        chi2 = float(((counts - N * p) ** 2 / (N * p)).sum())
        print("chi2 = %.3f" % chi2)
        assert chi2 < 40.790


class TestPlumbingCPU:
    def test_epsilon_ladder(self):
        e = ops.epsilon_ladder(8)
        assert e.dtype == torch.float32 and e.shape == (8,)
        assert float(e[0]) == pytest.approx(0.4, rel=1e-6)
        assert float(e[-1]) == pytest.approx(0.4 ** 8, rel=1e-6)
        assert bool((e[1:] < e[:-1]).all())
        assert ops.epsilon_ladder(1).tolist() == [pytest.approx(0.4, rel=1e-6)]
        e = ops.epsilon_ladder(3, base=0.5, alpha=1.0)
        assert e.tolist() == pytest.approx([0.5, 0.5 ** 1.5, 0.25], rel=1e-6)
        with pytest.raises(ValueError):
            ops.epsilon_ladder(0)

    def test_argument_errors(self):
        logits = torch.zeros(4, 3)
        u = torch.zeros(4, 2)
        state = ops.new_state(0)
        with pytest.raises(ValueError, match="exactly one"):
            ops.sample_categorical(logits, state=state, u=u)
        with pytest.raises(ValueError, match="exactly one"):
            ops.sample_categorical(logits)
        with pytest.raises(ValueError, match="exactly one"):
            ops.epsilon_greedy_dueling(torch.zeros(4), logits, 0.1, state=state, u=u)
        with pytest.raises(ValueError, match="exactly one"):
            ops.epsilon_greedy_dueling(torch.zeros(4), logits, 0.1)
        with pytest.raises(ValueError, match="A must be"):
            ops.sample_categorical(torch.zeros(2, 65), u=torch.zeros(2, 2))
        with pytest.raises(ValueError, match="A must be"):
            ops.epsilon_greedy_dueling(torch.zeros(2), torch.zeros(2, 65), 0.1,
                                       u=torch.zeros(2, 2))
        with pytest.raises(ValueError, match="float32"):
            ops.sample_categorical(logits.double(), u=u)
        with pytest.raises(ValueError, match="float32"):
            ops.sample_categorical(logits, u=u.double())
        with pytest.raises(ValueError, match="int64"):
            ops.sample_categorical(logits, state=state.to(torch.int32))
        with pytest.raises(ValueError, match=r"\[4, 2\]"):
            ops.sample_categorical(logits, u=torch.zeros(3, 2))
        with pytest.raises(ValueError, match="float32"):
            ops.epsilon_greedy_dueling(torch.zeros(4).double(), logits, 0.1, u=u)
        with pytest.raises(ValueError, match="float32"):
            ops.epsilon_greedy_dueling(torch.zeros(4), logits, torch.zeros(4).double(), u=u)
        with pytest.raises(ValueError, match="epsilons"):
            ops.epsilon_greedy_dueling(torch.zeros(4), logits, torch.zeros(3), u=u)
        assert state.tolist() == [0, 0]

    def test_atarinet_default_is_multinomial(self):
        from moolib_amd.models.atari import AtariNet

        torch.manual_seed(3)
        model = AtariNet(num_actions=6)
        assert model.sampler_state is None and model.sample_generator is None
        T, B = 2, 3
        inputs = atari_inputs(T, B, 6, "cpu")
        for state in (None, ops.new_state(1)):  # a state is ignored off the GPU
            model.sampler_state = state
            torch.manual_seed(5)
            with torch.no_grad():
                out, _ = model(inputs, tuple())
            torch.manual_seed(5)
            want = torch.multinomial(
                torch.softmax(out["policy_logits"].view(T * B, 6), dim=-1), num_samples=1
            ).view(T, B)
            assert torch.equal(out["action"], want)
        assert model.sampler_state.tolist() == [1, 0]

    def test_r2d2_act_default_is_unchanged(self):
        """A fixed-seed act() equals a copy of the code it had before the
        fused head, inlined here."""
        from moolib_amd.ops.r2d2 import dueling_q
        from moolib_amd.r2d2 import R2D2Config, R2D2Learner

        assert R2D2Config().fused_act is False
        learner, inputs, core = r2d2_learner("cpu", epsilon=0.5)
        assert learner.act_state is None
        torch.manual_seed(9)
        action, new_core = learner.act(inputs, core)
        torch.manual_seed(9)
        with torch.no_grad():
            out, want_core = learner.online(inputs, core)
            q = dueling_q(out["baseline"].float(), out["policy_logits"].float())
            want = q.argmax(dim=-1)
            explore = torch.rand(want.shape) < 0.5
            random_action = torch.randint_like(want, q.shape[-1])
            want = torch.where(explore, random_action, want)
        assert torch.equal(action, want)
        assert bool((action != q.argmax(dim=-1)).any()), "the case must explore"
        for a, b in zip(new_core, want_core):
            assert torch.equal(a, b)
        # return_q reports the same draw's Q-values
        torch.manual_seed(9)
        action2, _, (q_taken, q_max) = learner.act(inputs, core, return_q=True)
        assert torch.equal(action2, want)
        assert torch.equal(q_taken, q.gather(-1, want.unsqueeze(-1)).squeeze(-1))
        assert torch.equal(q_max, q.max(dim=-1).values)

    def test_r2d2_fused_act_cpu(self):
        check_r2d2_fused_act("cpu")

    def test_impala_flag(self, monkeypatch):
        from moolib_amd.impala import ImpalaConfig

        assert ImpalaConfig().fused_sampling is False
        monkeypatch.delenv("MOOLIB_AMD_FUSED_SAMPLING", raising=False)
        peer, broker = make_impala_peer("cpu")
        try:
            assert peer.cfg.fused_sampling is False
            assert peer._actor_sampler is None and peer._learn_sampler is None
            assert peer.fwd_model.sampler_state is None
            peer.act_once()
            assert peer.fwd_model.sampler_state is None
        finally:
            close_peer(peer)
        monkeypatch.setenv("MOOLIB_AMD_FUSED_SAMPLING", "1")
        peer, broker = make_impala_peer("cpu")
        try:
            assert peer.cfg.fused_sampling is True
            # no generator on the CPU today, so no state either
            assert peer._actor_sampler is None and peer._actor_rng is None
        finally:
            close_peer(peer)


# ----------------------------------------------------------------- helpers


def atari_inputs(T, B, A, device):
    g = torch.Generator().manual_seed(T * 100 + B)
    return {
        "state": torch.randint(0, 256, (T, B, 4, 84, 84), dtype=torch.uint8, generator=g).to(device),
        "reward": torch.randn(T, B, generator=g).to(device),
        "done": torch.zeros(T, B, dtype=torch.bool, device=device),
        "prev_action": torch.randint(0, A, (T, B), generator=g).to(device),
    }


class TinyNet(torch.nn.Module):
    """AtariNet's forward contract on a vector observation."""

    def __init__(self, num_actions=5):
        super().__init__()
        self.body = torch.nn.Linear(7, 16)
        self.policy = torch.nn.Linear(16, num_actions)
        self.baseline = torch.nn.Linear(16, 1)

    def initial_state(self, batch_size=1):
        return tuple()

    def forward(self, inputs, core_state=()):
        T, B = inputs["state"].shape[:2]
        x = torch.relu(self.body(inputs["state"].float()))
        out = dict(policy_logits=self.policy(x).float(), baseline=self.baseline(x).float().view(T, B))
        return out, core_state


def r2d2_learner(device, **cfg):
    from moolib_amd.r2d2 import R2D2Config, R2D2Learner

    torch.manual_seed(2)
    learner = R2D2Learner(TinyNet(), R2D2Config(**cfg), device, autocast=False)
    g = torch.Generator().manual_seed(4)
    inputs = {"state": torch.randn(3, 4, 7, generator=g).to(device)}
    return learner, inputs, tuple()


def check_r2d2_fused_act(device):
    from moolib_amd.ops.r2d2 import dueling_q

    learner, inputs, core = r2d2_learner(device, fused_act=True, seed=13, epsilon=0.5)
    assert learner.act_state.tolist() == [13, 0]
    with torch.no_grad():
        out, _ = learner.online(inputs, core)
    q = dueling_q(out["baseline"], out["policy_logits"])
    T, B, A = q.shape
    # an epsilon vector of zeros: the argmax, and q_taken == q_max
    default = torch.random.get_rng_state()
    action, _, (q_taken, q_max) = learner.act(
        inputs, core, epsilon=torch.zeros(B, device=device), return_q=True
    )
    assert torch.equal(torch.random.get_rng_state(), default), "no torch generator"
    assert action.shape == (T, B) and action.dtype == torch.int64
    assert torch.equal(action, q.argmax(dim=-1))
    assert torch.equal(q_taken, q_max)
    torch.testing.assert_close(q_max, q.max(dim=-1).values, rtol=1e-5, atol=1e-6)
    assert learner.act_state.tolist() == [13, 1]
    # a per-environment epsilon [B], broadcast over T, at the recorded step
    eps = torch.tensor([0.0, 1.0, 0.5, 1.0], device=device)
    action, _ = learner.act(inputs, core, epsilon=eps)
    u = ops.philox_uniforms(13, 1, T * B).to(device)
    want = ops.epsilon_greedy_dueling(
        out["baseline"], out["policy_logits"], eps.expand(T, B).contiguous(), u=u
    )[0]
    assert torch.equal(action, want)
    assert bool((action[:, 0] == q.argmax(dim=-1)[:, 0]).all())
    # the scalar of the config, without return_q
    action, _ = learner.act(inputs, core)
    u = ops.philox_uniforms(13, 2, T * B).to(device)
    want = ops.epsilon_greedy_dueling(out["baseline"], out["policy_logits"], 0.5, u=u)[0]
    assert torch.equal(action, want)
    assert learner.act_state.tolist() == [13, 3]


def make_impala_peer(device, **kw):
    import moolib_amd
    from moolib_amd.envs import SyntheticAtariEnv
    from moolib_amd.impala import ImpalaConfig, ImpalaPeer

    rpc = moolib_amd.Rpc()
    rpc.set_name("broker")
    broker = moolib_amd.Broker(rpc)
    addr = rpc.listen("127.0.0.1:0")[0]
    base = dict(num_actions=6, actor_batch_size=4, num_actor_batches=2, num_actor_cpus=2,
                batch_size=4, unroll_length=5, virtual_batch_size=4, device=device, connect=addr,
                total_steps=1e4, seed=3, autocast_bf16=device != "cpu")
    base.update(kw)
    peer = ImpalaPeer(ImpalaConfig(**base), lambda: SyntheticAtariEnv(num_actions=6), broker=broker)
    return peer, broker


def close_peer(peer):
    import gc

    for name in list(vars(peer)):
        setattr(peer, name, None)
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.synchronize()


# --------------------------------------------------------------------- GPU


def sentinels(N, device):
    return (torch.full((N,), -7, dtype=torch.int64, device=device),
            torch.full((N,), float("nan"), device=device),
            torch.full((N,), float("nan"), device=device))


@gpu
@requires_gpu
class TestKernels:
    @pytest.fixture(autouse=True)
    def _kernel_path(self, monkeypatch):
        monkeypatch.delenv("MOOLIB_AMD_NO_ACT_KERNEL", raising=False)
        assert ops._kernels() is not None

    @pytest.mark.parametrize("A", ACTIONS)
    @pytest.mark.parametrize("N", ROWS)
    def test_eps_greedy_equals_eager(self, N, A):
        value, adv, eps, u, ref = eps_greedy_case(N, A)
        eager = ops.epsilon_greedy_dueling(value, adv, eps, u=u)
        assert_eps_greedy(eager, ref)
        out = sentinels(N, "cuda")
        got = ops.epsilon_greedy_dueling(value.cuda(), adv.cuda(), eps.cuda(), u=u.cuda(), out=out)
        assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
        for g, e in zip(got, eager):
            assert torch.equal(g.cpu().view(torch.int32) if g.dtype == torch.float32 else g.cpu(),
                               e.view(torch.int32) if e.dtype == torch.float32 else e)

    @pytest.mark.parametrize("A", ACTIONS)
    @pytest.mark.parametrize("N", ROWS)
    def test_categorical_against_fp64(self, N, A):
        """Every row decidable under categorical_delta(A) must match the fp64
        reference; an undecidable one must return one of the two actions
        adjacent to its nearest boundary; at most 1% may be undecidable."""
        for scale in (1.0, 16.0):
            logits, u, (ref, margin, nearest) = logits_case(N, A, scale)
            out = torch.full((N,), -7, dtype=torch.int64, device="cuda")
            got = ops.sample_categorical(logits.cuda(), u=u.cuda(), out=out)
            assert got.data_ptr() == out.data_ptr()
            got = got.cpu().numpy()
            assert got.min() >= 0 and got.max() < A
            decidable = margin > categorical_delta(A)
            print("N=%d A=%d scale=%g undecidable=%d" % (N, A, scale, int((~decidable).sum())))
            assert np.array_equal(got[decidable], ref[decidable])
            near = ~decidable
            ok = (got[near] == nearest[near]) | (got[near] == np.minimum(nearest[near] + 1, A - 1))
            assert ok.all()
            assert near.sum() <= 0.01 * N

    @pytest.mark.parametrize("scale", [1.0, 4.0, 16.0])
    def test_categorical_4096_rows(self, scale):
        logits, u, (ref, margin, _) = logits_case(4096, 18, scale)
        assert int((margin <= categorical_delta(18)).sum()) == 0
        got = ops.sample_categorical(logits.cuda(), u=u.cuda())
        assert torch.equal(got.cpu(), torch.from_numpy(ref))

    @pytest.mark.parametrize("A", ACTIONS)
    def test_masked_logits_exact(self, A):
        logits, u, ref = masked_case(A)
        got = ops.sample_categorical(logits.cuda(), u=u.cuda()).cpu()
        assert torch.equal(got, ref)
        assert bool((logits.gather(1, got.unsqueeze(1)) == 0).all()), "a masked action"

    @pytest.mark.parametrize("seed,step", [(7, 0), (-1, (1 << 32) - 1), (1 << 40, 1 << 32)])
    @pytest.mark.parametrize("N,A", [(1, 1), (65, 3), (1025, 18), (2049, 64)])
    def test_state_equals_explicit_uniforms(self, N, A, seed, step):
        u = ops.philox_uniforms(seed, step, N).cuda()
        logits = logits_case(N, A, 4.0)[0].cuda()
        state = ops.new_state(seed, "cuda")
        state[1] = step
        got = ops.sample_categorical(logits, state=state)
        assert torch.equal(got, ops.sample_categorical(logits, u=u))
        assert state.tolist() == [ops.new_state(seed).tolist()[0], step + 1]

        value, adv, eps, _, _ = eps_greedy_case(N, A)
        value, adv, eps = value.cuda(), adv.cuda(), eps.cuda()
        state[1] = step
        got = ops.epsilon_greedy_dueling(value, adv, eps, state=state)
        want = ops.epsilon_greedy_dueling(value, adv, eps, u=u)
        for g, w in zip(got, want):
            assert torch.equal(g, w)
        assert int(state[1]) == step + 1

    def test_eager_path_on_the_gpu(self, monkeypatch):
        value, adv, eps, u, ref = eps_greedy_case(65, 18)
        monkeypatch.setenv("MOOLIB_AMD_NO_ACT_KERNEL", "1")
        state = ops.new_state(3, "cuda")
        got = ops.epsilon_greedy_dueling(value.cuda(), adv.cuda(), eps.cuda(), u=u.cuda())
        assert_eps_greedy(got, ref)
        ops.sample_categorical(adv.cuda(), state=state)
        assert state.tolist() == [3, 1]

    def test_kernel_rejects_bad_arguments(self):
        from moolib_amd import _kernels as k

        assert k.ACT_MAX_ACTIONS == ops.KERNEL_MAX_ACTIONS == 64
        x = torch.zeros(2, 65, device="cuda")
        with pytest.raises(RuntimeError, match="A must be"):
            k.act_categorical(x, None, torch.zeros(2, 2, device="cuda"))
        x = torch.zeros(2, 3, device="cuda")
        with pytest.raises(RuntimeError, match="exactly one"):
            k.act_categorical(x, None, None)
        with pytest.raises(RuntimeError, match="exactly one"):
            k.act_categorical(x, ops.new_state(0, "cuda"), torch.zeros(2, 2, device="cuda"))
        with pytest.raises(RuntimeError, match="u must be"):
            k.act_categorical(x, None, torch.zeros(3, 2, device="cuda"))

    def test_graph_replays_draw_fresh_numbers(self):
        N, A, seed, s = 672, 18, 99, 5
        logits = logits_case(N, A, 1.0)[0].cuda()
        state = ops.new_state(seed, "cuda")
        state[1] = s
        out = torch.full((N,), -7, dtype=torch.int64, device="cuda")
        ops.sample_categorical(logits, state=state, out=out)  # loads the code object
        state[1] = s
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ops.sample_categorical(logits, state=state, out=out)
        assert int(state[1]) == s, "a capture runs nothing"
        for i in range(3):
            g.replay()
            want = ops.sample_categorical(logits, u=ops.philox_uniforms(seed, s + i, N).cuda())
            assert torch.equal(out, want)
        assert state.tolist() == [seed, s + 3]


@gpu
@requires_gpu
class TestLearnersGPU:
    def test_atarinet_samples_with_its_state(self):
        from moolib_amd.models.atari import AtariNet

        torch.manual_seed(3)
        T, B, A = 2, 3, 18
        model = AtariNet(num_actions=A).cuda()
        model.sampler_state = ops.new_state(21, "cuda")
        model.sampler_state[1] = 8
        inputs = atari_inputs(T, B, A, "cuda")
        default = torch.cuda.get_rng_state()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            out, _ = model(inputs, tuple())
        assert torch.equal(torch.cuda.get_rng_state(), default), "no torch generator"
        assert model.sampler_state.tolist() == [21, 9]
        want = ops.sample_categorical(
            out["policy_logits"].view(T * B, A), u=ops.philox_uniforms(21, 8, T * B).cuda()
        )
        assert out["action"].shape == (T, B)
        assert torch.equal(out["action"].view(-1), want)

    def test_r2d2_fused_act(self):
        check_r2d2_fused_act("cuda")

    def test_impala_actor_graph_needs_no_generator(self):
        peer, broker = make_impala_peer("cuda", fused_sampling=True, prewarm=False)
        try:
            assert peer._actor_rng is None and peer._learn_rng is None
            assert peer._actor_sampler.tolist() == [7, 0]
            assert peer._learn_sampler.tolist() == [8, 0]
            assert peer._actor_call.generators == []
            for _ in range(5):  # three eager calls, the capture, one more replay
                peer.act_once()
            torch.cuda.synchronize()
            assert peer._actor_call.graph is not None, "the actor forward was not captured"
            assert peer.fwd_model.sampler_state is peer._actor_sampler
            # one draw per actor call, replays included
            assert peer._actor_sampler.tolist() == [7, 5]
            for step in (5, 6):
                peer.act_once()
                torch.cuda.synchronize()
                out = peer._actor_call.static_out["out"]
                logits = out["policy_logits"].float()
                B = logits.shape[1]
                want = ops.sample_categorical(
                    logits.view(B, -1), u=ops.philox_uniforms(7, step, B).cuda()
                )
                assert torch.equal(out["action"].view(-1), want)
                assert int(peer._actor_sampler[1]) == step + 1
        finally:
            close_peer(peer)
