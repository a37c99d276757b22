"""R2D2 learner (Kapturowski et al. 2019): a recurrent dueling double-Q
learner over replayed sequences.

Works with any model that follows AtariNet's forward contract
(`model(inputs, core_state) -> (out, core_state)` on time-major inputs, with
`out["baseline"]` [T,B] and `out["policy_logits"]` [T,B,A]): the unmodified
network acts as a dueling Q-network, `baseline` is V and `policy_logits` is
the advantage stream (ops.r2d2.dueling_q). The loss, its gradient and the
sequence priorities come from ops.r2d2.r2d2_loss — one fused HIP kernel on an
MI355X.
"""
import contextlib
import copy
import dataclasses

import torch

from moolib_amd.ops import act as act_ops
from moolib_amd.ops.r2d2 import dueling_q, r2d2_loss


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
