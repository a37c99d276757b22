"""float64 references and input generators for the R2D2 loss tests.

`r2d2_ref` is written from the definition with explicit loops over b, t and
i; `r2d2_ref_vectorised` reaches the same numbers by another route (the
Horner recursion R_j[t] = r_t + g_t R_{j-1}[t+1] over whole columns).
tests/test_r2d2.py checks one against the other without a GPU.
"""
import math

import torch

F64 = torch.float64


# ------------------------------------------------------------ value rescaling

def h(x, eps):
    return math.copysign(math.sqrt(abs(x) + 1.0) - 1.0, x) + eps * x


def h_inv(x, eps):
    """Cancellation-free inverse (valid for eps >= 0, including 0)."""
    a = abs(x) + 1.0 + eps
    s = 2.0 * a / (math.sqrt(1.0 + 4.0 * eps * a) + 1.0)
    return math.copysign(s * s - 1.0, x)


def h_inv_textbook(x, eps):
    """((sqrt(1 + 4 eps (|x|+1+eps)) - 1) / (2 eps))^2 - 1, eps > 0."""
    root = math.sqrt(1.0 + 4.0 * eps * (abs(x) + 1.0 + eps))
    return math.copysign(((root - 1.0) / (2.0 * eps)) ** 2 - 1.0, x)


# ------------------------------------------------------------------ reference

def _f64(case):
    return {
        k: (v.to(torch.int64) if k == "actions" else v.to(F64)) for k, v in case.items()
    }


def r2d2_ref(case, n, eps, rescale, eta, grad_scale=1.0):
    """Loops over b, t, i in float64. Returns a dict of float64 tensors:
    td [T,B], loss_seq [B], priority [B], grad_q [T,B,A], loss (scalar),
    tied [T,B] (the argmax row had more than one maximal element)."""
    c = _f64(case)
    q, qt, act = c["q"], c["q_target"], c["actions"]
    r, g, mask, w = c["rewards"], c["discounts"], c["mask"], c["is_weights"]
    T, B, A = q.shape
    fwd = (lambda x: h(x, eps)) if rescale else (lambda x: x)
    inv = (lambda x: h_inv(x, eps)) if rescale else (lambda x: x)
    td = torch.zeros(T, B, dtype=F64)
    grad_q = torch.zeros(T, B, A, dtype=F64)
    loss_seq = torch.zeros(B, dtype=F64)
    priority = torch.zeros(B, dtype=F64)
    tied = torch.zeros(T, B, dtype=torch.bool)
    for b in range(B):
        boot = []
        for s in range(T):
            row = q[s, b].tolist()
            best = max(row)
            a_star = row.index(best)  # lowest index wins ties
            tied[s, b] = row.count(best) > 1
            boot.append(inv(float(qt[s, b, a_star])))
        sum_sq = sum_abs = max_abs = n_valid = 0.0
        for t in range(T - 1):
            k = min(n, T - 1 - t)
            G, disc = 0.0, 1.0
            for i in range(k):
                G += disc * float(r[t + i, b])
                disc *= float(g[t + i, b])
            G += disc * boot[t + k]
            valid = float(mask[t, b])
            a_t = int(act[t, b])
            delta = valid * (fwd(G) - float(q[t, b, a_t]))
            td[t, b] = delta
            grad_q[t, b, a_t] = -grad_scale * float(w[b]) * delta
            sum_sq += delta * delta
            sum_abs += abs(delta)
            max_abs = max(max_abs, abs(delta))
            n_valid += valid
        loss_seq[b] = 0.5 * sum_sq
        priority[b] = eta * max_abs + (1.0 - eta) * sum_abs / max(1.0, n_valid)
    return {
        "td": td,
        "loss_seq": loss_seq,
        "priority": priority,
        "grad_q": grad_q,
        "loss": (w * loss_seq).mean(),
        "tied": tied,
    }


def r2d2_ref_vectorised(case, n, eps, rescale, eta, grad_scale=1.0):
    """Same quantities from whole-tensor float64 ops. R_0 = boot and
    R_j[t] = r_t + g_t R_{j-1}[t+1] for t < T-1 (R_j[T-1] stays boot[T-1]),
    so R_n[t] is the n-step return truncated at the end of the sequence."""
    c = _f64(case)
    q, qt, act = c["q"], c["q_target"], c["actions"]
    r, g, mask, w = c["rewards"], c["discounts"], c["mask"], c["is_weights"]
    T, B, A = q.shape

    def fwd(x):
        return torch.sign(x) * (torch.sqrt(x.abs() + 1) - 1) + eps * x if rescale else x

    def inv(x):
        if not rescale:
            return x
        a = x.abs() + 1 + eps
        s = 2 * a / (torch.sqrt(1 + 4 * eps * a) + 1)
        return torch.sign(x) * (s * s - 1)

    # first maximal index: the smallest j with q[j] == max
    is_max = q == q.max(dim=-1, keepdim=True).values
    idx = torch.arange(A).expand(T, B, A)
    a_star = torch.where(is_max, idx, torch.full_like(idx, A)).min(dim=-1).values
    boot = inv(qt.gather(-1, a_star.unsqueeze(-1)).squeeze(-1))
    R = boot.clone()
    for _ in range(n):
        R = torch.cat([r[:-1] + g[:-1] * R[1:], boot[-1:]], dim=0)
    valid = mask.clone()
    valid[-1] = 0
    qa = q.gather(-1, act.unsqueeze(-1)).squeeze(-1)
    td = valid * (fwd(R) - qa)
    td[-1] = 0
    loss_seq = 0.5 * (td * td).sum(0)
    priority = eta * td.abs().max(0).values + (1 - eta) * td.abs().sum(0) / valid.sum(0).clamp(min=1)
    grad_q = torch.zeros(T, B, A, dtype=F64)
    grad_q.scatter_(-1, act.unsqueeze(-1), (-grad_scale * w * td).unsqueeze(-1))
    return {
        "td": td,
        "loss_seq": loss_seq,
        "priority": priority,
        "grad_q": grad_q,
        "loss": (w * loss_seq).mean(),
    }


# ----------------------------------------------------------------- generators

def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randint(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g)


def int_case(seed, T, B, A, masked_columns=()):
    """Integer-exact inputs (rescale=False, n <= 5): q / q_target in -2..2,
    rewards in -3..3, discounts in {0, 0.5}, mask 0/1, is_weights 1. Every
    G_t is a multiple of 2^-5 below 2^5, so td, td^2 and their sums are exact
    in fp32 in any order. Each column's number of valid steps (mask over
    t < T-1) is 0 or a power of two, so the mean part of the priority is exact
    as well. Tensors are fp32 (int64 actions)."""
    g = _gen(seed)
    mask = torch.zeros(T, B)
    for b in range(B):
        if b in masked_columns or T < 2:
            continue
        choices = [0] + [1 << e for e in range(9) if (1 << e) <= T - 1]
        count = choices[int(_randint(g, (1,), 0, len(choices) - 1))]
        mask[torch.randperm(T - 1, generator=g)[:count], b] = 1.0
        mask[T - 1, b] = float(_randint(g, (1,), 0, 1))  # must be ignored
    return {
        "q": _randint(g, (T, B, A), -2, 2).float(),
        "q_target": _randint(g, (T, B, A), -2, 2).float(),
        "actions": _randint(g, (T, B), 0, A - 1),
        "rewards": _randint(g, (T, B), -3, 3).float(),
        "discounts": _randint(g, (T, B), 0, 1).float() * 0.5,
        "mask": mask,
        "is_weights": torch.ones(B),
    }


def float_case(seed, T, B, A, q_scale):
    """Random fp32 inputs: Q-values of scale `q_scale`, unit rewards, discount
    0.99 with 10% terminal steps, 80% of the steps unmasked, importance weights
    in (0.1, 1]."""
    g = _gen(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    ru = lambda *s: torch.rand(*s, generator=g)
    return {
        "q": rn(T, B, A) * q_scale,
        "q_target": rn(T, B, A) * q_scale,
        "actions": _randint(g, (T, B), 0, A - 1),
        "rewards": rn(T, B),
        "discounts": (ru(T, B) > 0.1).float() * 0.99,
        "mask": (ru(T, B) > 0.2).float(),
        "is_weights": 0.1 + 0.9 * ru(B),
    }
