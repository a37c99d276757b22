"""FlatAdam: torch.optim.Adam with gradient-norm clipping as ONE fused step
over flat buffers (ops.flat_adam: two HIP launches on an MI355X, plain torch
elsewhere).

The parameters, their gradients, the two moments and, if asked for, bf16
shadow copies of the parameters live in flat contiguous buffers; every
parameter and its `.grad` are views into them. The step counter and the
learning rate are device scalars, so `step()` never waits for the device and
can be captured by parallel.graphs.GraphedCall; a learning-rate scheduler
works unmodified, because `param_groups[0]["lr"]` is pushed to the device
scalar (one `fill_`, outside the kernels) whenever it has changed.

`state_dict()` / `load_state_dict()` use torch.optim.Adam's layout, so a
FlatAdam and an Adam can exchange their state in both directions.
"""
import torch

from moolib_amd.ops import flat_adam as _op

_ADAM_KEYS = ("step", "exp_avg", "exp_avg_sq")


def _flatten(params, dtype, with_grad):
    """Re-home `params` (and, with_grad, their .grad) as views of new flat
    buffers of `dtype`, the way impala.flatten_master_shadow does."""
    total = sum(p.numel() for p in params)
    dev = params[0].device
    flat = torch.empty(total, dtype=dtype, device=dev)
    grad = torch.zeros(total, dtype=dtype, device=dev) if with_grad else None
    off = 0
    with torch.no_grad():
        for p in params:
            n = p.numel()
            view = flat[off : off + n].view_as(p)
            view.copy_(p.detach())
            p.data = view
            if with_grad:
                gview = grad[off : off + n].view_as(p)
                if p.grad is not None:
                    gview.copy_(p.grad)
                p.grad = gview
            off += n
    return flat, grad


def _bump_versions(tensors):
    """The step writes through the flat buffers, which moves no parameter's
    version counter; version-keyed caches (ops/conv3x3's packed weights)
    must still see a change."""
    try:
        torch._C._increment_version(tensors)
    except TypeError:  # older torch: one tensor per call
        for t in tensors:
            torch._C._increment_version(t)


class FlatAdam(torch.optim.Optimizer):
    """Adam (no weight decay, amsgrad or maximize) with optional clipping of
    the global gradient norm to `max_grad_norm`, fused over flat buffers.

    One parameter group. Without `flat`, the parameters and their `.grad` are
    re-homed as views of new flat fp32 buffers (and `shadow_params`, bf16
    copies of the parameters in the same order, as views of a flat bf16
    buffer). With `flat = (flat_master, flat_grad32[, flat_shadow])` the
    optimizer adopts buffers the caller has laid out that way already
    (impala.flatten_master_shadow).

    `step()` returns the unclipped gradient norm as a 0-dim tensor that the
    next step overwrites. The gradients themselves are left unclipped.
    `zero_grad()` is one memset of the flat gradient and ALWAYS keeps
    `p.grad` a view of it, whatever `set_to_none` says: autograd and the
    Accumulator write through those views.
    """

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None,
                 shadow_params=None, flat=None, weight_decay=0.0, amsgrad=False, maximize=False):
        if weight_decay or amsgrad or maximize:
            raise ValueError("FlatAdam: weight_decay, amsgrad and maximize are not supported")
        if not lr >= 0.0:
            raise ValueError("FlatAdam: lr must be >= 0, got %r" % (lr,))
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("FlatAdam: betas must be in [0,1), got %r" % (betas,))
        if not eps >= 0.0:
            raise ValueError("FlatAdam: eps must be >= 0, got %r" % (eps,))
        if max_grad_norm is not None and not max_grad_norm > 0.0:
            raise ValueError("FlatAdam: max_grad_norm must be > 0 or None, got %r" % (max_grad_norm,))
        # the keys torch.optim.Adam keeps, so that either loads the other's state
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=0.0, amsgrad=False,
                        maximize=False)
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise ValueError("FlatAdam: exactly one parameter group, got %d" % len(self.param_groups))
        group = self.param_groups[0]
        if group["weight_decay"] or group["amsgrad"] or group["maximize"]:
            raise ValueError("FlatAdam: weight_decay, amsgrad and maximize are not supported")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        ps = group["params"]
        for p in ps:
            if p.dtype != torch.float32 or p.device != ps[0].device:
                raise ValueError("FlatAdam: parameters must be float32 on one device")
        self._params = list(ps)
        self._shadow_params = list(shadow_params) if shadow_params is not None else []
        if self._shadow_params and [s.shape for s in self._shadow_params] != [p.shape for p in ps]:
            raise ValueError("FlatAdam: shadow_params must match the parameters one to one")

        total = sum(p.numel() for p in ps)
        if flat is None:
            self._flat_p, self._flat_g = _flatten(ps, torch.float32, True)
            self._flat_shadow = None
            if self._shadow_params:
                self._flat_shadow, _ = _flatten(self._shadow_params, torch.bfloat16, False)
        else:
            self._flat_p, self._flat_g = flat[0], flat[1]
            self._flat_shadow = flat[2] if len(flat) > 2 else None
            off = 0
            for p in ps:  # the views must tile the buffers in parameter order
                want_p = self._flat_p.data_ptr() + 4 * off
                want_g = self._flat_g.data_ptr() + 4 * off
                if (p.data_ptr() != want_p or p.grad is None or p.grad.data_ptr() != want_g
                        or not p.is_contiguous() or not p.grad.is_contiguous()):
                    raise ValueError("FlatAdam: params and grads must be views tiling `flat` in order")
                off += p.numel()
            if self._flat_p.numel() != total or self._flat_g.numel() != total or (
                    self._flat_shadow is not None and self._flat_shadow.numel() != total):
                raise ValueError("FlatAdam: `flat` buffers must hold %d elements" % total)
        dev = self._flat_p.device
        self._m = torch.zeros(total, dtype=torch.float32, device=dev)
        self._v = torch.zeros(total, dtype=torch.float32, device=dev)
        self._step = torch.zeros((), dtype=torch.int64, device=dev)
        self._lr = torch.full((), float(group["lr"]), dtype=torch.float32, device=dev)
        self._lr_pushed = float(group["lr"])
        self._ws = _op.new_workspace(dev)
        self._touched = self._params + self._shadow_params

    # ------------------------------------------------------------------ step

    @torch.no_grad()
    def sync_lr(self):
        """Push `param_groups[0]["lr"]` to the device scalar if it has changed
        (one `fill_`, no host wait). `step()` does this itself, except while a
        graph is being captured: a captured fill would reset lr to the value at
        capture on every replay, and a replay runs no Python at all. Whoever
        replays a captured `step()` calls this before each replay; betas, eps
        and max_grad_norm are baked into a capture."""
        lr = float(self.param_groups[0]["lr"])
        if lr != self._lr_pushed:
            self._lr.fill_(lr)
            self._lr_pushed = lr

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            with torch.enable_grad():
                closure()
        group = self.param_groups[0]
        if not (self._flat_p.is_cuda and torch.cuda.is_current_stream_capturing()):
            self.sync_lr()
        beta1, beta2 = group["betas"]
        norm = _op.flat_adam_step(
            self._flat_p, self._flat_g, self._m, self._v, self._step, self._lr, beta1, beta2,
            group["eps"], shadow=self._flat_shadow, max_norm=self.max_grad_norm,
            workspace=self._ws,
        )
        _bump_versions(self._touched)
        return norm

    def zero_grad(self, set_to_none=True):
        """One memset of the flat gradient. `p.grad` stays a view of the flat
        buffer whatever `set_to_none` says."""
        self._flat_g.zero_()

    # ----------------------------------------------------------------- state

    def _views(self, flat):
        out, off = [], 0
        for p in self._params:
            out.append(flat[off : off + p.numel()].view_as(p))
            off += p.numel()
        return out

    def state_dict(self):
        """torch.optim.Adam's layout: per-parameter `step` (fp32 scalar on the
        host, as a non-capturable Adam keeps it), `exp_avg`, `exp_avg_sq`."""
        step = float(self._step.item())
        state = {
            i: {"step": torch.tensor(step), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
            for i, (m, v) in enumerate(zip(self._views(self._m), self._views(self._v)))
        }
        group = {k: v for k, v in self.param_groups[0].items() if k != "params"}
        group["params"] = list(range(len(self._params)))
        return {"state": state, "param_groups": [group]}

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """Copies into the flat buffers; the parameter views stay."""
        groups = state_dict["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self._params):
            raise ValueError("FlatAdam: the state must hold one group of %d parameters"
                             % len(self._params))
        saved = groups[0]
        if saved.get("weight_decay") or saved.get("amsgrad") or saved.get("maximize"):
            raise ValueError("FlatAdam: weight_decay, amsgrad and maximize are not supported")
        state = state_dict["state"]
        steps = set()
        for pid, m, v in zip(saved["params"], self._views(self._m), self._views(self._v)):
            s = state.get(pid)
            if not s:  # a parameter Adam has not stepped yet
                m.zero_()
                v.zero_()
                steps.add(0)
                continue
            m.copy_(s["exp_avg"])
            v.copy_(s["exp_avg_sq"])
            steps.add(int(float(s["step"])))
        if len(steps) != 1:
            raise ValueError("FlatAdam: parameters at different steps %r" % sorted(steps))
        self._step.fill_(steps.pop())
        group = self.param_groups[0]
        for k, val in saved.items():
            if k != "params" and k in group:
                group[k] = tuple(val) if k == "betas" else val
        self._lr.fill_(float(group["lr"]))
        self._lr_pushed = float(group["lr"])
