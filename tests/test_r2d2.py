"""R2D2 loss: references, eager path, learner (CPU) and the fused kernel (GPU).

docs/KERNEL_TESTS.md ("R2D2 loss") has the arguments and the recorded figures.

* The float64 reference `r2d2_refs.r2d2_ref` (explicit loops) is checked
  against a second, vectorised float64 formulation.
* Integer-exact cases (rescale off, small-integer inputs, discounts 0 / 0.5):
  every output is exactly representable, so the fp32 eager path and the kernel
  must be `torch.equal` to the reference.
* Float cases: the kernel's error against float64 is bounded by
  4 * max(e_ref, 2^-24 * scale), where e_ref is the error of the eager fp32
  CPU path on the same inputs (computed here, never taken from the kernel),
  and every element stays within 1e-4 + 1e-5 |ref|.
* A one-state MDP whose fixed point h(2) pins the semantics (window, rescaling,
  bootstrap index), on the eager path and through the kernel.
"""
import functools
import json

import pytest
import torch

import r2d2_refs as R
from moolib_amd.ops import r2d2 as ops

gpu = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

EPS = 1e-3
MAX_T = ops.KERNEL_MAX_T

# (T, B, A, n): no valid step; the smallest real one; n beyond the sequence;
# odd sizes; more than one block; A at and across the wave width (64); the
# kernel's T limit (column 0 fully masked there).
SHAPES = [
    (1, 1, 1, 1), (2, 1, 1, 1), (2, 3, 2, 5), (5, 3, 6, 3), (9, 5, 4, 5), (7, 65, 18, 5),
    (4, 2, 64, 2), (4, 2, 65, 2), (3, 2, 130, 1), (MAX_T, 2, 3, 4),
]
Q_SCALES = [1.0, 30.0]
TENSORS = ("td", "loss_seq", "priority", "grad_q")


def _figure(**kw):
    """One machine-readable line per measured figure (shown with pytest -s)."""
    print("KERNEL_EDGES_FIGURE " + json.dumps(kw))


def _seed(shape):
    T, B, A, n = shape
    return 1000 * T + 100 * B + 10 * A + n


@functools.lru_cache(maxsize=None)
def int_case(shape):
    T, B, A, _ = shape
    return R.int_case(_seed(shape), T, B, A, masked_columns=(0,) if T == MAX_T else ())


@functools.lru_cache(maxsize=None)
def int_ref(shape, eta):
    return R.r2d2_ref(int_case(shape), shape[3], 0.0, False, eta, grad_scale=1.0)


@functools.lru_cache(maxsize=None)
def float_case(shape, q_scale):
    T, B, A, _ = shape
    case = R.float_case(_seed(shape) + int(q_scale), T, B, A, q_scale)
    if T == MAX_T:
        case["mask"][:, 0] = 0.0
    return case


@functools.lru_cache(maxsize=None)
def float_ref(shape, q_scale):
    """float64 reference with grad_scale = 1/B (what the op passes)."""
    return R.r2d2_ref(float_case(shape, q_scale), shape[3], EPS, True, 0.9,
                      grad_scale=1.0 / shape[1])


def eager_outputs(case, n, eps, rescale, eta):
    """The fp32 eager path on the CPU: td, loss_seq, priority, loss and the
    autograd gradient of `loss` w.r.t. q (its grad_scale is 1/B)."""
    q = case["q"].clone().requires_grad_(True)
    out = ops.r2d2_loss(q, case["q_target"], case["actions"], case["rewards"],
                        case["discounts"], case["mask"], case["is_weights"],
                        n_step=n, eps=eps, rescale=rescale, eta=eta)
    out.loss.backward()
    return {"td": out.td_errors, "loss_seq": out.loss_per_sequence,
            "priority": out.priorities, "grad_q": q.grad, "loss": out.loss.detach()}


@functools.lru_cache(maxsize=None)
def float_eager(shape, q_scale):
    return eager_outputs(float_case(shape, q_scale), shape[3], EPS, True, 0.9)


def older_tolerance(ref):
    return 1e-4 + 1e-5 * ref.abs()


def within(got, ref, bound):
    """max|got - ref| <= bound (scalar) and every element within the older
    tolerance; returns the error."""
    err = (got.double().cpu() - ref).abs()
    assert bool((err <= older_tolerance(ref)).all()), float(err.max())
    worst = float(err.max()) if err.numel() else 0.0
    assert worst <= bound, (worst, bound)
    return worst


def kernel_bound(e_ref, ref):
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    return 4.0 * max(e_ref, 2.0 ** -24 * scale)


# =============================================================== CPU tests


class TestReferences:
    @pytest.mark.parametrize("shape", SHAPES)
    def test_loop_reference_matches_vectorised(self, shape):
        n = shape[3]
        for case, args in [
            (float_case(shape, 1.0), (n, EPS, True, 0.9, 0.37)),
            (float_case(shape, 30.0), (n, 0.0, True, 0.25, 1.0)),
            (int_case(shape), (n, 0.0, False, 0.0, 1.0)),
        ]:
            a, b = R.r2d2_ref(case, *args), R.r2d2_ref_vectorised(case, *args)
            for name in TENSORS + ("loss",):
                assert torch.allclose(a[name], b[name], rtol=1e-12, atol=1e-12), name

    def test_rescale_round_trip_fp64(self):
        x = torch.linspace(-50, 50, 4001, dtype=torch.float64)
        for eps in (1e-3, 1e-2, 0.0):
            back = ops.value_rescale(ops.inverse_value_rescale(x, eps), eps)
            assert float((back - x).abs().max()) <= 1e-12
            mine = torch.tensor([R.h(R.h_inv(v, eps), eps) for v in x.tolist()], dtype=R.F64)
            assert float((mine - x).abs().max()) <= 1e-12
            inv = torch.tensor([R.h_inv(v, eps) for v in x.tolist()], dtype=R.F64)
            # two float64 codings of one formula (values up to 2400): a few ulp
            assert torch.allclose(ops.inverse_value_rescale(x, eps), inv, rtol=1e-14, atol=0)

    def test_stable_and_textbook_inverse_agree_fp64(self):
        for v in torch.linspace(-50, 50, 4001, dtype=torch.float64).tolist():
            assert abs(R.h_inv(v, EPS) - R.h_inv_textbook(v, EPS)) <= 1e-10

    def test_rescale_off_is_identity(self):
        case = int_case((5, 3, 6, 3))
        a = R.r2d2_ref(case, 3, 0.0, False, 1.0)
        b = eager_outputs(case, 3, 0.123, False, 1.0)  # eps must be ignored
        assert torch.equal(b["td"].double(), a["td"])

    def test_dueling_q(self):
        v = torch.tensor([[1.0, -2.0]])
        adv = torch.tensor([[[1.0, 2.0, 6.0], [0.0, 0.0, 3.0]]])
        want = torch.tensor([[[-1.0, 0.0, 4.0], [-3.0, -3.0, 0.0]]])
        assert torch.equal(ops.dueling_q(v, adv), want)


class TestEager:
    @pytest.mark.parametrize("q_scale", Q_SCALES)
    @pytest.mark.parametrize("shape", SHAPES)
    def test_float_case_against_fp64(self, shape, q_scale):
        ref, got = float_ref(shape, q_scale), float_eager(shape, q_scale)
        for name in TENSORS + ("loss",):
            err = (got[name].double() - ref[name]).abs()
            assert bool((err <= older_tolerance(ref[name])).all()), (name, float(err.max()))

    @pytest.mark.parametrize("shape", SHAPES)
    def test_autograd_gradient_is_the_analytic_one(self, shape):
        """d loss / d q from ordinary autograd against -grad_scale w delta at
        a_t. The gradient is w/B times a TD error, so it inherits the TD
        error's tolerance scaled by w/B, plus a few fp32 roundings."""
        T, B, A, _ = shape
        case, ref, got = float_case(shape, 1.0), float_ref(shape, 1.0), float_eager(shape, 1.0)
        taken = torch.zeros(T, B, A, dtype=torch.bool)
        taken.scatter_(-1, case["actions"].unsqueeze(-1), True)
        assert torch.equal(got["grad_q"][~taken], torch.zeros(int((~taken).sum())))
        w = (case["is_weights"].double() / B).view(1, B, 1)
        bound = w * older_tolerance(ref["td"]).unsqueeze(-1) + 4 * 2.0 ** -24 * ref["grad_q"].abs()
        assert bool(((got["grad_q"].double() - ref["grad_q"]).abs() <= bound).all())

    def test_noncontiguous_and_int32_inputs(self):
        shape = (5, 3, 6, 3)
        case, want = float_case(shape, 1.0), float_eager(shape, 1.0)
        q = case["q"].transpose(0, 1).contiguous().transpose(0, 1).requires_grad_(True)
        assert not q.is_contiguous()
        out = ops.r2d2_loss(q, case["q_target"], case["actions"].to(torch.int32),
                            case["rewards"], case["discounts"], case["mask"],
                            case["is_weights"], n_step=3, eps=EPS, eta=0.9)
        out.loss.backward()
        assert torch.equal(out.td_errors, want["td"])
        assert torch.equal(q.grad, want["grad_q"])

    def test_rejects_bad_scalars(self):
        case = int_case((2, 1, 1, 1))
        args = [case[k] for k in ("q", "q_target", "actions", "rewards", "discounts", "mask",
                                  "is_weights")]
        for kw in ({"n_step": 0}, {"eps": -1e-3}, {"eta": 1.5}):
            with pytest.raises(ValueError):
                ops.r2d2_loss(*args, **kw)


class TestIntegerPremise:
    @pytest.mark.parametrize("shape", SHAPES)
    def test_reference_values_are_exact_in_fp32(self, shape):
        """td is a multiple of 2^-5, td^2 of 2^-10; the sums stay below 2^24
        of those units, and the valid count is 0 or a power of two."""
        case = int_case(shape)
        assert shape[3] <= 5
        for eta in (0.0, 1.0):
            ref = int_ref(shape, eta)
            for name, unit in (("td", 2.0 ** 5), ("grad_q", 2.0 ** 5), ("loss_seq", 2.0 ** 11)):
                scaled = ref[name] * unit
                assert torch.equal(scaled, scaled.round()), name
                assert float(scaled.abs().max()) < 2 ** 24, name
                assert torch.equal(ref[name].float().double(), ref[name]), name
            assert float(ref["td"].abs().sum(0).max()) * 2 ** 5 < 2 ** 24
            assert torch.equal(ref["priority"].float().double(), ref["priority"])
        count = case["mask"][:-1].sum(0)
        assert all(c == 0 or (c & (c - 1)) == 0 for c in count.long().tolist())

    def test_ties_are_common(self):
        ref = int_ref((9, 5, 4, 5), 1.0)
        assert float(ref["tied"].float().mean()) >= 0.25
        many = int_ref((7, 65, 18, 5), 1.0)
        assert float(many["tied"].float().mean()) >= 0.25

    @pytest.mark.parametrize("eta", [0.0, 1.0])
    @pytest.mark.parametrize("shape", SHAPES)
    def test_eager_fp32_equals_reference(self, shape, eta):
        ref = int_ref(shape, eta)
        got = eager_outputs(int_case(shape), shape[3], 0.0, False, eta)
        for name in ("td", "loss_seq", "priority"):
            assert torch.equal(got[name].double(), ref[name]), name

    def test_eager_gradient_equals_reference(self):
        shape = (6, 4, 5, 3)  # B a power of two: grad_scale 1/B is exact
        case = R.int_case(7, 6, 4, 5)
        ref = R.r2d2_ref(case, 3, 0.0, False, 1.0, grad_scale=0.25)
        got = eager_outputs(case, 3, 0.0, False, 1.0)
        assert torch.equal(got["grad_q"].double(), ref["grad_q"])
        assert float(ref["grad_q"].abs().max()) > 0


# ------------------------------------------------------------- fixed point


def fixed_point_run(device, steps=100):
    """One state, two actions, reward 1, gamma 0.5, never terminating: both
    Q-values must converge to h(G*) with G* = 1 + 1/2 + 1/4 + G*/8 = 2."""
    T, B, n = 6, 4, 3
    theta = torch.zeros(2, device=device, requires_grad=True)
    t_idx = torch.arange(T, device=device).view(T, 1)
    b_idx = torch.arange(B, device=device).view(1, B)
    actions = (t_idx + b_idx) % 2
    ones = torch.ones(T, B, device=device)
    out = None
    for _ in range(steps):
        q = theta.expand(T, B, 2)
        out = ops.r2d2_loss(q, theta.detach().expand(T, B, 2), actions, ones, 0.5 * ones, ones,
                            torch.ones(B, device=device), n_step=n, eps=EPS, eta=0.9)
        (grad,) = torch.autograd.grad(out.loss, theta)
        with torch.no_grad():
            theta -= 0.2 * grad
    return theta.detach().cpu(), out.priorities.cpu()


H_OF_2 = 0.7340508  # sqrt(3) - 1 + 2e-3


def check_fixed_point(theta, priorities):
    assert abs(R.h(2.0, EPS) - H_OF_2) < 5e-8
    assert float((theta.double() - R.h(2.0, EPS)).abs().max()) <= 1e-5
    assert float(priorities.abs().max()) <= 1e-5


def test_fixed_point_eager():
    check_fixed_point(*fixed_point_run("cpu"))


# ----------------------------------------------------------------- learner


class TinyNet(torch.nn.Module):
    """Stand-in with AtariNet's forward contract: [T,B,4] float state, an LSTM
    core reset where done, policy_logits / baseline heads."""

    def __init__(self, num_actions=3):
        super().__init__()
        self.num_actions = num_actions
        self.fc = torch.nn.Linear(4 + 1 + num_actions, 8)
        self.core = torch.nn.LSTM(8, 8)
        self.policy = torch.nn.Linear(8, num_actions)
        self.baseline = torch.nn.Linear(8, 1)

    def initial_state(self, batch_size=1):
        return tuple(torch.zeros(1, batch_size, 8) for _ in range(2))

    def forward(self, inputs, core_state):
        T, B = inputs["reward"].shape
        onehot = torch.nn.functional.one_hot(inputs["prev_action"], self.num_actions).float()
        x = torch.cat([inputs["state"], inputs["reward"].unsqueeze(-1), onehot], dim=-1)
        x = torch.relu(self.fc(x))
        outs = []
        for t in range(T):
            nd = (~inputs["done"][t]).float().view(1, B, 1)
            core_state = tuple(nd * s for s in core_state)
            o, core_state = self.core(x[t:t + 1], core_state)
            outs.append(o)
        y = torch.cat(outs)
        out = {"policy_logits": self.policy(y), "baseline": self.baseline(y).squeeze(-1)}
        return out, core_state


def tiny_batch(T=7, B=3, A=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    return {
        "state": torch.randn(T, B, 4, generator=g),
        "reward": torch.randn(T, B, generator=g),
        "done": torch.rand(T, B, generator=g) < 0.15,
        "prev_action": torch.randint(0, A, (T, B), generator=g),
        "action": torch.randint(0, A, (T, B), generator=g),
        "core_state": tuple(0.1 * torch.randn(1, B, 8, generator=g) for _ in range(2)),
    }


class TestLearnerCPU:
    def make(self, **kw):
        from moolib_amd.r2d2 import R2D2Config, R2D2Learner

        torch.manual_seed(0)
        return R2D2Learner(TinyNet(), R2D2Config(lr=1e-2, **kw), "cpu")

    def test_learn_returns_priorities_and_masks_burn_in(self, monkeypatch):
        import moolib_amd.r2d2 as mod

        seen = {}

        def spy(*args, **kw):
            seen["mask"] = args[5]
            seen["out"] = ops.r2d2_loss(*args, **kw)
            return seen["out"]

        monkeypatch.setattr(mod, "r2d2_loss", spy)
        learner = self.make(burn_in=2, n_step=3)
        before = [p.detach().clone() for p in learner.online.parameters()]
        metrics, prio = learner.learn(tiny_batch(), torch.ones(3))
        assert prio.shape == (3,) and bool(torch.isfinite(prio).all())
        assert bool(torch.isfinite(metrics["loss"])) and float(metrics["mean_abs_td"]) > 0
        td = seen["out"].td_errors
        assert torch.equal(td[:2], torch.zeros(2, 3)) and torch.equal(td[-1], torch.zeros(3))
        assert float(td[2:-1].abs().min()) > 0
        assert torch.equal(seen["mask"][:2], torch.zeros(2, 3))
        assert any(not torch.equal(a, b.detach())
                   for a, b in zip(before, learner.online.parameters()))

    def test_rewards_and_discounts_follow_the_action(self, monkeypatch):
        import moolib_amd.r2d2 as mod

        seen = {}

        def spy(*args, **kw):
            seen["rewards"], seen["discounts"] = args[3], args[4]
            return ops.r2d2_loss(*args, **kw)

        monkeypatch.setattr(mod, "r2d2_loss", spy)
        batch = tiny_batch()
        self.make(discount=0.9).learn(batch, torch.ones(3))
        assert torch.equal(seen["rewards"][:-1], batch["reward"][1:])
        assert torch.equal(seen["discounts"][:-1], 0.9 * (~batch["done"][1:]).float())

    def test_target_syncs_exactly_at_the_interval(self):
        learner = self.make(target_update_interval=3)
        initial = [p.detach().clone() for p in learner.target.parameters()]

        def target_is(params):
            return all(torch.equal(a, b.detach())
                       for a, b in zip(learner.target.parameters(), params))

        for step in range(1, 7):
            learner.learn(tiny_batch(seed=step), torch.ones(3))
            if step % 3 == 0:
                assert target_is(list(learner.online.parameters())), step
                initial = [p.detach().clone() for p in learner.target.parameters()]
            else:
                assert target_is(initial), step
                assert not target_is(list(learner.online.parameters())), step

    def test_act_greedy_is_argmax_of_dueling_q(self):
        learner = self.make(epsilon=0.0)
        batch = tiny_batch(T=1, B=5)
        inputs = {k: batch[k] for k in ("state", "reward", "done", "prev_action")}
        action, state = learner.act(inputs, batch["core_state"])
        with torch.no_grad():
            out, want_state = learner.online(inputs, batch["core_state"])
        q = ops.dueling_q(out["baseline"], out["policy_logits"])
        assert torch.equal(action, q.argmax(-1)) and action.shape == (1, 5)
        assert all(torch.equal(a, b) for a, b in zip(state, want_state))

    def test_act_explores(self):
        learner = self.make(epsilon=1.0)
        batch = tiny_batch(T=1, B=64)
        inputs = {k: batch[k] for k in ("state", "reward", "done", "prev_action")}
        action, _ = learner.act(inputs, batch["core_state"])
        assert set(action.unique().tolist()) == {0, 1, 2}


# =============================================================== GPU tests


def kernel_call(case, n, eps, rescale, eta, grad_scale, nan_fill=True):
    """The raw kernel on the GPU, writing grad_q into a NaN-filled buffer."""
    from moolib_amd import _kernels

    dev = {k: v.cuda() for k, v in case.items()}
    grad_out = torch.full(case["q"].shape, float("nan"), device="cuda") if nan_fill else None
    td, loss_seq, priority, grad_q = _kernels.r2d2_loss(
        dev["q"], dev["q_target"], dev["actions"], dev["rewards"], dev["discounts"],
        dev["mask"], dev["is_weights"], n, eps, rescale, eta, grad_scale, grad_out)
    if nan_fill:
        assert grad_q.data_ptr() == grad_out.data_ptr()
    return {"td": td, "loss_seq": loss_seq, "priority": priority, "grad_q": grad_q}


@gpu
@requires_gpu
class TestKernel:
    def test_limit_matches_the_op(self):
        from moolib_amd import _kernels

        assert _kernels.R2D2_MAX_T == MAX_T >= 128

    @pytest.mark.parametrize("eta", [0.0, 1.0])
    @pytest.mark.parametrize("shape", SHAPES)
    def test_integer_exact(self, shape, eta):
        ref = int_ref(shape, eta)
        got = kernel_call(int_case(shape), shape[3], 0.0, False, eta, 1.0)
        for name in TENSORS:
            assert torch.equal(got[name].cpu().double(), ref[name]), name
        if shape[0] == 1:
            assert all(not bool(got[name].any()) for name in TENSORS)

    @pytest.mark.parametrize("q_scale", Q_SCALES)
    @pytest.mark.parametrize("shape", SHAPES)
    def test_float_case(self, shape, q_scale):
        ref, eager = float_ref(shape, q_scale), float_eager(shape, q_scale)
        got = kernel_call(float_case(shape, q_scale), shape[3], EPS, True, 0.9, 1.0 / shape[1])
        taken = torch.zeros(shape[:3], dtype=torch.bool)
        taken.scatter_(-1, float_case(shape, q_scale)["actions"].unsqueeze(-1), True)
        assert not bool(got["grad_q"].cpu()[~taken].any())  # exactly 0, no NaN left
        for name in TENSORS:
            e_ref = float((eager[name].double() - ref[name]).abs().max())
            bound = kernel_bound(e_ref, ref[name])
            err = float((got[name].cpu().double() - ref[name]).abs().max())
            _figure(test="r2d2_loss", case="%d %d %d %d %g" % (shape + (q_scale,)),
                    tensor=name, e_ref=e_ref, err=err, bound=bound)
            within(got[name], ref[name], bound)

    def test_bit_reproducible(self):
        shape = (7, 65, 18, 5)
        case = float_case(shape, 30.0)
        a = kernel_call(case, 5, EPS, True, 0.9, 1.0 / 65)
        b = kernel_call(case, 5, EPS, True, 0.9, 1.0 / 65, nan_fill=False)
        for name in TENSORS:
            assert torch.equal(a[name], b[name]), name

    def test_out_of_range_actions_are_clamped(self):
        shape = (5, 3, 6, 3)
        case = dict(int_case(shape))
        bad = case["actions"].clone()
        bad[1, 0], bad[2, 1] = 6, -1
        zeroed = case["actions"].clone()
        zeroed[1, 0], zeroed[2, 1] = 0, 0
        got = kernel_call(dict(case, actions=bad), 3, 0.0, False, 1.0, 1.0)
        want = kernel_call(dict(case, actions=zeroed), 3, 0.0, False, 1.0, 1.0)
        for name in TENSORS:
            assert torch.equal(got[name], want[name]), name

    def test_autograd_int32_actions_transposed_q(self):
        shape, q_scale = (7, 65, 18, 5), 1.0
        case, ref, eager = float_case(shape, q_scale), float_ref(shape, q_scale), \
            float_eager(shape, q_scale)
        q = case["q"].cuda().transpose(0, 1).contiguous().transpose(0, 1).requires_grad_(True)
        assert not q.is_contiguous()
        out = ops.r2d2_loss(q, case["q_target"].cuda(), case["actions"].cuda().to(torch.int32),
                            case["rewards"].cuda(), case["discounts"].cuda(),
                            case["mask"].cuda(), case["is_weights"].cuda(),
                            n_step=5, eps=EPS, eta=0.9)
        (3.0 * out.loss).backward()
        got = {"loss": out.loss.detach(), "grad_q": q.grad / 3.0, "td": out.td_errors,
               "priority": out.priorities, "loss_seq": out.loss_per_sequence}
        for name in ("loss", "grad_q", "td", "priority", "loss_seq"):
            e_ref = float((eager[name].double() - ref[name]).abs().max())
            bound = kernel_bound(e_ref, ref[name])
            err = within(got[name], ref[name], bound)
            _figure(test="r2d2_loss_autograd", tensor=name, e_ref=e_ref, err=err, bound=bound)

    def test_env_switch_selects_the_eager_path(self, monkeypatch):
        shape = (5, 3, 6, 3)
        case = {k: v.cuda() for k, v in float_case(shape, 1.0).items()}
        args = [case[k] for k in ("q", "q_target", "actions", "rewards", "discounts", "mask",
                                  "is_weights")]
        fused = ops.r2d2_loss(*args, n_step=3)
        monkeypatch.setenv("MOOLIB_AMD_NO_R2D2_KERNEL", "1")
        eager = ops.r2d2_loss(*args, n_step=3)
        assert torch.allclose(fused.td_errors, eager.td_errors, atol=1e-5)
        assert torch.allclose(fused.priorities, eager.priorities, atol=1e-5)

    def test_host_checks(self):
        from moolib_amd import _kernels

        T, B, A = 4, 2, 3
        good = {k: v.cuda() for k, v in R.float_case(1, T, B, A, 1.0).items()}
        order = ("q", "q_target", "actions", "rewards", "discounts", "mask", "is_weights")

        def call(n=2, eps=EPS, **override):
            a = dict(good, **override)
            return _kernels.r2d2_loss(*[a[k] for k in order], n, eps, True, 0.9, 1.0)

        call()
        bad = [
            dict(q=good["q"].double()),
            dict(actions=good["actions"].int()),
            dict(mask=good["mask"].bool()),
            dict(rewards=good["rewards"].cpu()),
            dict(q=good["q"].cpu()),
            dict(q_target=good["q_target"][:, :, :2].contiguous()),
            dict(discounts=good["discounts"][:3].contiguous()),
            dict(is_weights=torch.ones(B + 1, device="cuda")),
            dict(q_target=good["q_target"].transpose(0, 1).contiguous().transpose(0, 1)),
            dict(n=0),
            dict(eps=-1.0),
        ]
        for kw in bad:
            with pytest.raises(RuntimeError, match="r2d2_loss"):
                call(**kw)
        long = {k: v.cuda() for k, v in R.float_case(2, MAX_T + 1, 1, 2, 1.0).items()}
        with pytest.raises(RuntimeError, match="limit"):
            _kernels.r2d2_loss(*[long[k] for k in order], 2, EPS, True, 0.9, 1.0)
        with pytest.raises(RuntimeError, match="grad_out"):
            _kernels.r2d2_loss(*[good[k] for k in order], 2, EPS, True, 0.9, 1.0,
                               torch.empty(T, B, A + 1, device="cuda"))

    def test_fixed_point_through_the_kernel(self):
        check_fixed_point(*fixed_point_run("cuda"))


@gpu
@requires_gpu
def test_learner_gpu_atarinet_lstm_and_replay_round_trip():
    from moolib_amd.models.atari import AtariNet
    from moolib_amd.r2d2 import R2D2Config, R2D2Learner
    from moolib_amd.replay import ReplayBuffer

    torch.manual_seed(0)
    T, B, A = 6, 2, 18
    model = AtariNet(num_actions=A, use_lstm=True)
    learner = R2D2Learner(model, R2D2Config(burn_in=2, n_step=3), "cuda", autocast=True)
    buf = ReplayBuffer(8, device="cuda")
    for i in range(4):  # one item per sequence, core state included
        buf.add({
            "state": torch.randint(0, 256, (T, 4, 84, 84), dtype=torch.uint8),
            "reward": torch.randn(T),
            "done": torch.zeros(T, dtype=torch.bool),
            "prev_action": torch.randint(0, A, (T,)),
            "action": torch.randint(0, A, (T,)),
            "core_h": 0.1 * torch.randn(1, 256),
            "core_c": 0.1 * torch.randn(1, 256),
        })
    items, idx, w = buf.sample(B)
    batch = {k: items[k].transpose(0, 1) for k in ("state", "reward", "done", "prev_action",
                                                  "action")}
    batch["core_state"] = (items["core_h"].transpose(0, 1), items["core_c"].transpose(0, 1))
    before = [p.detach().clone() for p in learner.online.parameters()]
    metrics, prio = learner.learn(batch, w)
    assert prio.is_cuda and prio.shape == (B,)
    assert bool(torch.isfinite(prio).all()) and bool(torch.isfinite(metrics["loss"]))
    assert float(metrics["mean_abs_td"]) > 0
    assert any(not torch.equal(a, b.detach())
               for a, b in zip(before, learner.online.parameters()))
    buf.update_priorities(idx, prio)
    want = prio.clamp_min(1e-6) ** buf.alpha
    assert torch.equal(buf.priorities[idx[-1]], want[-1])
    items, idx, w = buf.sample(B)
    assert bool(torch.isfinite(w).all()) and items["state"].shape == (B, T, 4, 84, 84)
