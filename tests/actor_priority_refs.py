"""float64 reference and input generators for the actor-priority tests.

`actor_priority_ref` is written from the definition in docs/KERNEL_TESTS.md
("Actor priorities") with explicit loops over the environment k, the step t
and the window index i, in numpy float64. It shares no code with
moolib_amd/ops/r2d2.py.
"""
import math

import numpy as np


def h(x, eps):
    return math.copysign(math.sqrt(abs(x) + 1.0) - 1.0, x) + eps * x


def h_inv(x, eps):
    """Cancellation-free inverse of h (valid for eps >= 0, including 0)."""
    a = abs(x) + 1.0 + eps
    s = 2.0 * a / (math.sqrt(1.0 + 4.0 * eps * a) + 1.0)
    return math.copysign(s * s - 1.0, x)


def actor_priority_ref(case, n_step, discount, eps, rescale, eta, burn_in):
    """Returns (priority [K], td [T, K]) as float64 arrays. `case` holds
    q_taken, q_max, reward (float) and done (0/1) as [T, K] arrays in the
    actor's layout: reward[t], done[t] arrive with step t. `discount` is taken
    at the precision the op uses it (fp32)."""
    q_taken = np.asarray(case["q_taken"], dtype=np.float64)
    q_max = np.asarray(case["q_max"], dtype=np.float64)
    reward = np.asarray(case["reward"], dtype=np.float64)
    done = np.asarray(case["done"]) != 0
    gamma = float(np.float32(discount))
    T, K = q_taken.shape
    td = np.zeros((T, K), dtype=np.float64)
    priority = np.zeros(K, dtype=np.float64)
    for k in range(K):
        boot = [h_inv(float(q_max[s, k]), eps) if rescale else float(q_max[s, k])
                for s in range(T)]
        sum_abs = max_abs = n_valid = 0.0
        for t in range(T - 1):
            steps = min(n_step, T - 1 - t)
            G, disc = 0.0, 1.0
            for i in range(steps):
                G = G + disc * float(reward[t + i + 1, k])
                disc = disc * (0.0 if done[t + i + 1, k] else gamma)
            G = G + disc * boot[t + steps]
            valid = 1.0 if t >= burn_in else 0.0
            delta = valid * ((h(G, eps) if rescale else G) - float(q_taken[t, k]))
            td[t, k] = delta
            sum_abs += abs(delta)
            max_abs = max(max_abs, abs(delta))
            n_valid += valid
        priority[k] = eta * max_abs + (1.0 - eta) * sum_abs / max(1.0, n_valid)
    return priority, td


# ----------------------------------------------------------------- generators


def int_case(seed, T, K, A=4):
    """Integer-exact inputs (rescale off, discount 0.5, n <= 5): q [T, K, A]
    integers in -2..2 and random actions give q_taken <= q_max in -2..2;
    rewards in -3..3; 20% terminal steps. Every return is a multiple of 2^-5
    below 2^5, so every TD error and every sum of them is exact in fp32."""
    rng = np.random.RandomState(seed)
    q = rng.randint(-2, 3, size=(T, K, A)).astype(np.float32)
    actions = rng.randint(0, A, size=(T, K))
    return {
        "q": q,
        "actions": actions,
        "q_taken": np.take_along_axis(q, actions[..., None], axis=-1)[..., 0],
        "q_max": q.max(axis=-1),
        "reward": rng.randint(-3, 4, size=(T, K)).astype(np.float32),
        "done": (rng.rand(T, K) < 0.2),
    }


def float_case(seed, T, K, q_scale):
    """Q-values of scale `q_scale` (q_max >= q_taken), unit-normal rewards, 10%
    terminal steps."""
    rng = np.random.RandomState(seed)
    a = (rng.randn(T, K) * q_scale).astype(np.float32)
    b = (rng.randn(T, K) * q_scale).astype(np.float32)
    return {
        "q_taken": np.minimum(a, b),
        "q_max": np.maximum(a, b),
        "reward": rng.randn(T, K).astype(np.float32),
        "done": (rng.rand(T, K) < 0.1),
    }
