"""R2D2 learner (Kapturowski et al. 2019): a recurrent dueling double-Q
learner over replayed sequences.

Works with any model that follows AtariNet's forward contract
(`model(inputs, core_state) -> (out, core_state)` on time-major inputs, with
`out["baseline"]` [T,B] and `out["policy_logits"]` [T,B,A]): the unmodified
network acts as a dueling Q-network, `baseline` is V and `policy_logits` is
the advantage stream (ops.r2d2.dueling_q). The loss, its gradient and the
sequence priorities come from ops.r2d2.r2d2_loss — one fused HIP kernel on an
MI355X. On the actor's side, SequenceBuilder cuts the stream of steps into
overlapping sequences and gives each its initial priority.
"""
import collections
import contextlib
import copy
import dataclasses

import torch

from moolib_amd.ops import act as act_ops
from moolib_amd.ops.r2d2 import actor_priorities, dueling_q, r2d2_loss


@dataclasses.dataclass
class R2D2Config:
    n_step: int = 5
    burn_in: int = 0  # leading steps that only warm up the recurrent state
    eps: float = 1e-3  # value-rescaling epsilon
    eta: float = 0.9  # priority = eta max|td| + (1-eta) mean|td|
    discount: float = 0.997
    target_update_interval: int = 100  # learner steps between target syncs
    lr: float = 1e-4
    grad_clip: float = 40.0
    epsilon: float = 0.01  # exploration rate of act()
    fused_optimizer: bool = False  # clip + Adam as one fused flat step (optim.FlatAdam)
    fused_act: bool = False  # act() head as one fused launch (ops.act.epsilon_greedy_dueling)
    seed: int = None  # of the fused act head's sampler state; None takes a fresh one


class SequenceBuilder:
    """Cuts an actor's stream of steps into replay sequences of `unroll` steps
    that start every `period` steps (R2D2: unroll 80, period 40), each with
    the recurrent state at its own start and, given the act head's Q-values,
    its initial priority (ops.r2d2.actor_priorities).

        b = SequenceBuilder(unroll, period)            # period None: disjoint
        out = b.append(step, core_state, q_taken, q_max)

    `step` is a dict of [K, ...] tensors with at least `reward` and `done`;
    `core_state` is the (h, c) tuple [1, K, H] the network held BEFORE it
    consumed this step, or () for a model without a core; `q_taken` / `q_max`
    are [K] or [1, K]. `append` returns None until a window is complete, then
    (items, priorities): every leaf stacked [unroll, K, ...], `core_h` /
    `core_c` of the window's first step if there is a core, and priorities
    [K] (None if no Q-values are given). Sequence j covers the global steps
    [j * period, j * period + unroll).

    Emitted tensors are the builder's window buffers, handed over: the next
    window starts in fresh ones that receive the last `unroll - period` rows,
    so nothing emitted is written again and source and destination of the tail
    copy never overlap. The recurrent state is cloned at every step whose
    index is a multiple of `period` (the caller's tensors may be the static
    outputs of a captured graph). Nothing is read back to the host.
    """

    _Q_KEYS = ("q_taken", "q_max")

    def __init__(self, unroll, period=None, n_step=5, discount=0.997, eps=1e-3, eta=0.9,
                 burn_in=0):
        self.unroll = int(unroll)
        self.period = self.unroll if period is None else int(period)
        if self.unroll < 1:
            raise ValueError("SequenceBuilder: unroll must be >= 1, got %d" % self.unroll)
        if not 1 <= self.period <= self.unroll:
            raise ValueError("SequenceBuilder: period must be in [1, unroll = %d], got %d"
                             % (self.unroll, self.period))
        self.priority_args = dict(n_step=n_step, discount=discount, eps=eps, eta=eta,
                                  burn_in=burn_in)
        self.num_envs = None
        self.with_q = None
        self.window = None  # leaf name -> [unroll, K, ...]; the Q rows under _Q_KEYS
        self.q_window = None
        self.fill = 0  # rows of the window that are written
        self.step_index = 0  # global index of the next step
        self.starts = collections.deque()  # core states of the sequences not yet emitted

    def _check(self, step, core_state, q):
        for key in ("reward", "done"):
            if key not in step:
                raise ValueError("SequenceBuilder.append: step has no %r" % key)
        for key in ("core_h", "core_c"):
            if key in step:
                raise ValueError("SequenceBuilder.append: %r is the builder's own key" % key)
        K = step["reward"].shape[0]
        if self.num_envs is None:
            self.num_envs, self.with_q = K, q is not None
        if len(core_state) not in (0, 2):
            raise ValueError("SequenceBuilder.append: core_state must be (h, c) or ()")
        for name, t in list(step.items()) + [("q", t) for t in (q or ())]:
            if t.dim() < 1 or t.shape[0] != self.num_envs:
                raise ValueError("SequenceBuilder.append: %s has shape %s, expected %d environments"
                                 % (name, tuple(t.shape), self.num_envs))
        for s in core_state:
            if s.dim() != 3 or s.shape[1] != self.num_envs:
                raise ValueError("SequenceBuilder.append: core state of shape %s, expected "
                                 "[1, %d, H]" % (tuple(s.shape), self.num_envs))
        if (q is not None) != self.with_q:
            raise ValueError("SequenceBuilder.append: Q-values must come with every step or none")
        if self.window is not None and set(step) != set(self.window):
            raise ValueError("SequenceBuilder.append: step keys %s, expected %s"
                             % (sorted(step), sorted(self.window)))

    def _fresh(self, rows):
        return {k: t.new_empty((self.unroll,) + tuple(t.shape)) for k, t in rows.items()}

    @torch.no_grad()
    def append(self, step, core_state=(), q_taken=None, q_max=None):
        if (q_taken is None) != (q_max is None):
            raise ValueError("SequenceBuilder.append: q_taken and q_max come together")
        q = None
        if q_taken is not None:
            q = tuple(t.reshape(-1) if t.dim() == 2 and t.shape[0] == 1 else t
                      for t in (q_taken, q_max))
        self._check(step, core_state, q)
        q_rows = dict(zip(self._Q_KEYS, q)) if q is not None else {}
        if self.window is None:
            self.window, self.q_window = self._fresh(step), self._fresh(q_rows)
        if self.step_index % self.period == 0:
            self.starts.append(tuple(s.clone() for s in core_state))
        for window, rows in ((self.window, step), (self.q_window, q_rows)):
            for k, t in rows.items():
                window[k][self.fill].copy_(t, non_blocking=True)
        self.fill += 1
        self.step_index += 1
        if self.fill < self.unroll:
            return None

        items, q_items = self.window, self.q_window
        keep = self.unroll - self.period
        self.window, self.q_window = self._fresh(step), self._fresh(q_rows)
        for new, old in ((self.window, items), (self.q_window, q_items)):
            for k in new:
                new[k][:keep].copy_(old[k][self.period:])
        self.fill = keep
        priorities = None
        if self.with_q:
            device = q_items["q_taken"].device
            priorities = actor_priorities(
                q_items["q_taken"], q_items["q_max"], items["reward"].to(device),
                items["done"].to(device), **self.priority_args
            ).priorities
        start = self.starts.popleft()
        items = dict(items)
        if start:
            items["core_h"], items["core_c"] = start
        return items, priorities


class R2D2Learner:
    """Owns an online and a target copy of `model` and the optimizer."""

    def __init__(self, model, config=None, device="cpu", autocast=None):
        self.config = config or R2D2Config()
        self.device = torch.device(device)
        self.online = model.to(self.device)
        self.target = copy.deepcopy(self.online)
        for p in self.target.parameters():
            p.requires_grad_(False)
        if self.config.fused_optimizer:
            from moolib_amd.optim import FlatAdam

            self.optimizer = FlatAdam(
                self.online.parameters(), lr=self.config.lr, eps=1e-3,
                max_grad_norm=self.config.grad_clip,
            )
        else:
            self.optimizer = torch.optim.Adam(
                self.online.parameters(), lr=self.config.lr, eps=1e-3
            )
        # bf16 autocast is what routes AtariNet onto the MFMA kernels
        self.autocast = (self.device.type == "cuda") if autocast is None else bool(autocast)
        self.steps = 0
        # [seed, step] of the fused act head; lives with the model
        self.act_state = None
        if self.config.fused_act:
            seed = self.config.seed
            if seed is None:
                seed = int(torch.seed()) % (2**62)
            self.act_state = act_ops.new_state(seed, self.device)

    def _amp(self):
        if self.autocast:
            return torch.autocast(self.device.type, dtype=torch.bfloat16)
        return contextlib.nullcontext()

    def _q_values(self, model, inputs, core_state):
        with self._amp():
            out, core_state = model(inputs, core_state)
        return dueling_q(out["baseline"].float(), out["policy_logits"].float()), core_state

    @torch.no_grad()
    def act(self, inputs, core_state, epsilon=None, return_q=False):
        """epsilon-greedy actions [T,B] for time-major `inputs`, and the new
        core state.

        `epsilon`, a float32 [B] tensor of one exploration rate per
        environment, overrides config.epsilon. With `return_q` the result is
        (action, core_state, (q_taken, q_max)): the Q-values of the actions
        taken and of the greedy ones, each [T,B]. With config.fused_act the
        whole head is one launch of ops.act.epsilon_greedy_dueling driven by
        the learner's own sampler state, and no torch generator is used.
        """
        if self.config.fused_act:
            with self._amp():
                out, core_state = self.online(inputs, core_state)
            value = out["baseline"].float()
            eps = self.config.epsilon if epsilon is None else (
                epsilon.to(value.device).expand(value.shape)
            )
            action, q_taken, q_max = act_ops.epsilon_greedy_dueling(
                value, out["policy_logits"].float(), eps, state=self.act_state
            )
            if return_q:
                return action, core_state, (q_taken, q_max)
            return action, core_state
        q, core_state = self._q_values(self.online, inputs, core_state)
        greedy = action = q.argmax(dim=-1)
        if epsilon is not None or self.config.epsilon > 0:
            eps = self.config.epsilon if epsilon is None else epsilon.to(action.device)
            explore = torch.rand(action.shape, device=action.device) < eps
            random_action = torch.randint_like(action, q.shape[-1])
            action = torch.where(explore, random_action, action)
        if return_q:
            taken = q.gather(-1, action.unsqueeze(-1)).squeeze(-1)
            return action, core_state, (taken, q.gather(-1, greedy.unsqueeze(-1)).squeeze(-1))
        return action, core_state

    def sequence_builder(self, unroll, period=None):
        """A SequenceBuilder whose priorities use this learner's n_step,
        discount, eps, eta and burn_in, i.e. the ones `learn` will return for
        the same sequence while the target network equals the online one."""
        cfg = self.config
        return SequenceBuilder(unroll, period, n_step=cfg.n_step, discount=cfg.discount,
                               eps=cfg.eps, eta=cfg.eta, burn_in=cfg.burn_in)

    def sync_target(self):
        self.target.load_state_dict(self.online.state_dict())

    def learn(self, batch, is_weights):
        """One optimizer step on a time-major batch of sequences.

        `batch` holds state, reward, done, prev_action, action ([T,B,...], in
        the actor's layout: reward[t] and done[t] arrive WITH state[t]) and
        `core_state`, the recurrent state stored at the start of each sequence
        (absent: the model's initial state). The first `burn_in` steps run
        through the same forward but carry no loss (mask 0). Returns
        (metrics, priorities): metrics are 0-dim tensors (no host sync here),
        priorities [B] live on the batch's device, ready for
        ReplayBuffer.update_priorities.
        """
        cfg = self.config
        # a replay sample is batch-major; its time-major transpose is a view
        move = lambda t: t.to(self.device).contiguous()
        batch = {
            k: (tuple(move(s) for s in v) if k == "core_state" else move(v))
            for k, v in batch.items()
        }
        T, B = batch["reward"].shape
        core_state = batch.get("core_state")
        if core_state is None:
            core_state = tuple(s.to(self.device) for s in self.online.initial_state(B))
        inputs = {k: batch[k] for k in ("state", "reward", "done", "prev_action")}

        # The loss wants r_t and gamma_t to FOLLOW a_t: they arrive with the
        # next state. The last step has no successor; it only bootstraps.
        last = torch.zeros(1, B, device=self.device)
        rewards = torch.cat([batch["reward"][1:].float(), last], dim=0)
        discounts = torch.cat([cfg.discount * (~batch["done"][1:].bool()).float(), last], dim=0)
        mask = torch.ones(T, B, device=self.device)
        mask[: cfg.burn_in] = 0.0

        q, _ = self._q_values(self.online, inputs, core_state)
        with torch.no_grad():
            q_target, _ = self._q_values(self.target, inputs, core_state)
        out = r2d2_loss(
            q, q_target, batch["action"], rewards, discounts, mask,
            torch.as_tensor(is_weights, dtype=torch.float32, device=self.device),
            n_step=cfg.n_step, eps=cfg.eps, rescale=True, eta=cfg.eta,
        )
        self.optimizer.zero_grad(set_to_none=True)
        out.loss.backward()
        if cfg.fused_optimizer:
            # the fused step forms the norm and clips; the norm tensor is the
            # optimizer's own and the next step overwrites it
            grad_norm = self.optimizer.step().clone()
        else:
            grad_norm = torch.nn.utils.clip_grad_norm_(self.online.parameters(), cfg.grad_clip)
            self.optimizer.step()
        self.steps += 1
        if self.steps % cfg.target_update_interval == 0:
            self.sync_target()

        n_valid = mask[:-1].sum().clamp(min=1.0)
        metrics = {
            "loss": out.loss.detach(),
            "mean_abs_td": out.td_errors.abs().sum() / n_valid,
            "grad_norm": grad_norm.detach(),
        }
        return metrics, out.priorities
