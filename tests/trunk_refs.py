"""Float64 CPU reference of the whole AtariNet with bf16 rounding points
(tests/test_trunk_composed.py; docs/KERNEL_TESTS.md, "Composed trunk").

The network is re-implemented from its definition out of the references in
tests/kernel_refs.py: 3 x (conv -> 3x3/2 max-pool -> 2 residual blocks), ReLU,
FC, clipped reward and one-hot action, optional LSTM, two heads. Gradients
come from autograd. One extra primitive, `Q`, rounds to bf16 in the forward
pass and rounds the gradient that flows back through it to bf16:

* `R_exact` is the reference with every `Q` switched off (`rounding(False,
  False)`);
* `R_emul` has a `Q` wherever the GPU path materialises a bf16 tensor or hands
  autograd a bf16 gradient. Which gradients are bf16 depends on the dtype of
  the parameters, hence `mode`: "a" is bf16 shadow weights (ImpalaPeer's
  fwd_model), "b" fp32 master weights under bf16 autocast (R2D2Learner); and
  on where the conv weight gradient comes from, hence `wgrad`: "kernel" is the
  project's fp32 kernel (its sum is cast to the weight's dtype), "wrw" MIOpen's
  weight-gradient convolution (it returns bf16).

A value feeding two consumers gets the sum of two bf16 gradients, formed in
bf16: the `Q` on the value rounds that sum, the `Q`s on the consumers' inputs
round the two terms.
"""
import contextlib

import numpy as np
import torch

import kernel_refs as R

F64 = torch.float64
CHANS = (16, 32, 32)
FRAME_SCALE = float(np.float32(1.0 / 255.0))

# ------------------------------------------------------------------ Q

_state = {"act": True, "param": True}
_probe = None


@contextlib.contextmanager
def rounding(act=True, param=True):
    """Switch the activation / activation-gradient `Q`s and the parameter /
    parameter-gradient `Q`s. Both off is R_exact."""
    old = dict(_state)
    _state.update(act=act, param=param)
    try:
        yield
    finally:
        _state.update(old)


@contextlib.contextmanager
def probing():
    """Collect the premise figures of the integer-exact test while a reference
    runs: the largest |value| and |gradient| seen by an activation `Q`, the
    largest sum of |terms| of any fp32 sum the GPU path forms, the largest
    |parameter gradient| before its cast, how many of all these are not
    integers, and the fewest channels left alive by any ReLU."""
    global _probe
    old = _probe
    _probe = {"act_max": 0.0, "grad_max": 0.0, "sum_max": 0.0, "pgrad_max": 0.0, "nonint": 0,
              "live_min": 1 << 30}
    try:
        yield _probe
    finally:
        _probe = old


def _note(key, t):
    if _probe is None or t.numel() == 0:
        return
    _probe[key] = max(_probe[key], t.detach().abs().max().item())
    _probe["nonint"] += int((t.detach() != t.detach().round()).sum().item())


class _QFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kind, fwd, bwd):
        ctx.kind, ctx.bwd = kind, bwd
        if kind == "act":
            _note("act_max", x)
        return R.bf16_round(x) if fwd else x.clone()

    @staticmethod
    def backward(ctx, g):
        _note("grad_max" if ctx.kind == "act" else "pgrad_max", g)
        return (R.bf16_round(g) if ctx.bwd else g), None, None, None


def Q(x, kind="act", fwd=True, bwd=True):
    """bf16 round-to-nearest-even of the value (fwd) and of the gradient that
    comes back (bwd); the identity when `kind` is switched off."""
    if not _state[kind] or not (fwd or bwd):
        return x
    return _QFn.apply(x, kind, fwd, bwd)


# ------------------------------------------------------------------ ops


def _probe_conv(x, w, y):
    """Sums of |terms| of the forward, dgrad, wgrad and bias-gradient sums."""
    if _probe is None:
        return
    xd, wd = x.detach(), w.detach()
    _note("sum_max", R.conv3x3_abs_ref(xd, wd))

    def hook(g):
        ga = g.detach().abs()
        _note("sum_max", R.conv3x3_wgrad_ref(xd.abs(), ga))
        _note("sum_max", R.conv3x3_dgrad_ref(ga, wd.abs()))
        _note("sum_max", ga.sum(dim=(0, 2, 3)))

    if y.requires_grad:
        y.register_hook(hook)


def conv(x, w, dw_rounds, bias=None):
    """3x3 conv, output rounded; `dy` is rounded by the output's Q, `dx` by
    the Q on the input, `dW` when the path returns it in bf16. `bias` is the
    first conv's fused epilogue bias (one rounding for conv + bias)."""
    y = R.conv3x3_ref(Q(x), Q(w, "param", fwd=False, bwd=dw_rounds))
    _probe_conv(x, w, y)
    if bias is not None:
        y = y + bias.view(1, -1, 1, 1)
    return Q(y)


def maxpool(x):
    """max_pool2d(x, 3, 2, 1) with maxpool3x3s2_ref's tie rule (the first
    maximum in row-major scan order of the window wins) in both directions:
    the `where` chain routes the gradient to the tap that was selected."""
    N, C, H, W = x.shape
    OH, OW = (H + 1) // 2, (W + 1) // 2
    xp = x.new_full((N, C, 2 * OH + 1, 2 * OW + 1), float("-inf"))
    xp[:, :, 1 : H + 1, 1 : W + 1] = x
    best = None
    for kh in range(3):
        for kw in range(3):
            v = xp[:, :, kh : kh + 2 * OH - 1 : 2, kw : kw + 2 * OW - 1 : 2]
            best = v if best is None else torch.where(v > best, v, best)
    return best


def relu(x):
    y = torch.relu(x)
    if _probe is not None:  # channels of the producing conv that are live somewhere
        live = int((y.detach() > 0).any(0).flatten(1).any(1).sum())
        _probe["live_min"] = min(_probe["live_min"], live)
    return y


def bias_relu(x, b):
    """relu(x + b) in one pass: one rounding; db is an fp32 sum cast to the
    bf16 bias the op was handed."""
    return Q(relu(x + Q(b, "param").view(1, -1, 1, 1)))


def bias_add2(x, b1, s, b2=None, b2_grad=True):
    if b2 is not None and not b2_grad:
        b2 = b2.detach()
    y = x + Q(b1, "param").view(1, -1, 1, 1) + s
    if b2 is not None:
        y = y + Q(b2, "param").view(1, -1, 1, 1)
    return Q(y)


def linear(x, w, b):
    """bf16 GEMM with the bias in its epilogue: output, dx, dW and db are all
    bf16 tensors, whatever the parameters' dtype."""
    return Q(Q(x) @ Q(w, "param").t() + Q(b, "param"))


def residual_block(x, p, pre, dw_rounds, pending=None, mutate=()):
    t = bias_relu(x, pending) if pending is not None else relu(x)
    u = conv(t, p[pre + "conv0.weight"], dw_rounds)
    t = bias_relu(u, p[pre + "conv0.bias"])
    u = conv(t, p[pre + "conv1.weight"], dw_rounds)
    return bias_add2(u, p[pre + "conv1.bias"], x, None if "drop_bias2" in mutate else pending,
                     b2_grad="no_b2_grad" not in mutate)


def lstm_plain(X, h0, c0, w, nd):
    """kernel_refs.lstm_exact's recurrence, left to autograd."""
    h, c = h0, c0
    Hs = []
    for t in range(X.shape[0]):
        m = nd[t].unsqueeze(-1)
        h, c = h * m, c * m
        i, f, g, o = (X[t] + h @ w.t()).chunk(4, dim=-1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        Hs.append(h)
    return torch.stack(Hs), h, c


class _LstmEmulFn(torch.autograd.Function):
    """kernel_refs.lstm_emul (forward and hand-written backward with the
    kernel's rounding points) as one autograd node."""

    @staticmethod
    def forward(ctx, X, h0, c0, w, nd, rounding_on, round_g, dw_unshifted):
        z = torch.zeros
        d = {"X": X, "h0": h0, "c0": c0, "w": w, "nd": nd,
             "gH": z(X.shape[0], X.shape[1], h0.shape[1], dtype=F64),
             "ghT": z(h0.shape, dtype=F64), "gcT": z(h0.shape, dtype=F64)}
        out = R.lstm_emul(d, rounding_on, round_g)
        ctx.d, ctx.flags, ctx.H = d, (rounding_on, round_g), out["H"]
        ctx.dw_unshifted = dw_unshifted
        return out["H"], out["hT"], out["cT"]

    @staticmethod
    def backward(ctx, gH, ghT, gcT):
        out = R.lstm_emul(dict(ctx.d, gH=gH, ghT=ghT, gcT=gcT), *ctx.flags)
        dW = out["dW"]
        if ctx.dw_unshifted:  # the mutation: dG[t]^T @ H[t] where H[t-1] belongs
            dW = torch.einsum("tbg,tbh->gh", out["dX"], ctx.H)
        return out["dX"], out["dh0"], out["dc0"], dW, None, None, None, None


def lstm(X, h0, c0, w, nd, force_emul=False, round_g=True, dw_unshifted=False):
    """lstm_emul when the activation Qs are on, else the plain recurrence;
    `force_emul` runs lstm_emul with its rounding off instead (the two must
    then agree). `round_g=False` leaves G = X + hW unrounded, as the 128 / 512
    kernels do. `dw_unshifted` is a mutation of lstm_emul's backward."""
    if _state["act"] or force_emul or dw_unshifted:
        return _LstmEmulFn.apply(X, h0, c0, w, nd, _state["act"], round_g, dw_unshifted)
    return lstm_plain(X, h0, c0, w, nd)


def fc_relu(flat, w, b, fused=False):
    """relu(fc(flat)) on `flat`, the relu'd trunk output. Default route: the
    bf16 GEMM of `linear`, then relu (a selection, no rounding). `fused`
    (ops/fc.py::trunk_fc, hip/fc.hip.inc): fp32 sum, bias and relu, one
    rounding; d_x rounded once; dW and db stay fp32 sums (no Q of their own).
    The values agree: rounding commutes with relu, in both directions."""
    if fused:
        return Q(torch.relu(Q(flat, fwd=False) @ w.t() + b))
    return torch.relu(linear(flat, w, b))


def core_input_proj(feat, reward, action, w, b_ih, b_hh, fused=False, mutate=()):
    """The LSTM's input projection Xg [M,4H] from feat [M,F], reward [M],
    prev_action [M], weight_ih_l0 [4H, F+1+A] (columns: features, reward,
    actions) and both biases.

    Default route (models/atari.py: clamp, one_hot, cat, F.linear): the clamped
    reward is cast to bf16, the bias sum is rounded, the GEMM is bf16 (output,
    dx, dW, db all rounded). `fused` (ops/lstm.py::core_input_projection,
    hip/lstm_input.hip.inc): reward clamped in fp32 and not rounded, biases
    added in fp32, one rounding of Xg; d_feat rounded once; dW and db are fp32
    sums. Mutations: reward_unclamped, action_shifted."""
    M, F_ = feat.shape
    A = w.shape[1] - F_ - 1
    r = reward.reshape(M).to(F64)
    if "reward_unclamped" not in mutate:
        r = r.clamp(-1, 1)
    if not fused:
        r = Q(r)
    extra = torch.zeros(M, 1 + A, dtype=F64)
    extra[:, 0] = r
    first = 0 if "action_shifted" in mutate else 1
    extra[torch.arange(M), first + action.reshape(M).long()] += 1.0
    if fused:
        return Q(Q(feat, fwd=False) @ w[:, :F_].t() + extra @ w[:, F_:].t() + b_ih + b_hh)
    return linear(torch.cat([feat, extra], dim=-1), w, b_ih + b_hh)


# ------------------------------------------------------------------ the net

SECTION_PARAMS = tuple(
    "sections.%d.%s.%s" % (s, m, k)
    for s in range(3)
    for m in ("conv", "res0.conv0", "res0.conv1", "res1.conv0", "res1.conv1")
    for k in ("weight", "bias")
)


def decode_frames(x_u8):
    """uint8 [N,4,H,W] -> x * scale as the frames kernel computes it (fp32
    product, TestFramesExact), then rounded to bf16."""
    return Q((x_u8.float() * torch.tensor(FRAME_SCALE, dtype=torch.float32)).double())


def trunk(frames_u8, p, mode, wgrad, mutate=()):
    """The three conv sections as AtariNet.forward wires them on the GPU: the
    first conv takes the u8 frames and has its bias in the epilogue (weight
    gradient always from the project's kernel); the other two section convs
    run bias-free and their bias rides through the pool into res0 as a
    pending bias. Returns relu(x) flattened in NCHW order, [N, 3872]."""
    top_rounds = mode == "a"  # .grad has the parameter's dtype
    p = {k: Q(v, "param", fwd=True, bwd=top_rounds) for k, v in p.items()}
    dw_rounds = mode == "a" or wgrad == "wrw"
    x = decode_frames(frames_u8)
    for s in range(3):
        pre = "sections.%d." % s
        w, b = p[pre + "conv.weight"], p[pre + "conv.bias"]
        if s == 0:
            x = Q(maxpool(conv(x, w, mode == "a", bias=b)))
            pending = None
        else:
            x = Q(maxpool(conv(x, w, dw_rounds)))
            pending = b
        x = residual_block(x, p, pre + "res0.", dw_rounds, pending, mutate)
        x = residual_block(x, p, pre + "res1.", dw_rounds)
    x = relu(x)
    if "flatten_nhwc" in mutate:
        return x.permute(0, 2, 3, 1).reshape(x.shape[0], -1)
    return x.reshape(x.shape[0], -1)


def trunk_graph(params, frames_u8, mode="a", wgrad="kernel", mutate=()):
    """The trunk's forward, kept with its autograd graph, so that several
    networks that share frames and section parameters (the core cases of
    three widths) pay for it once: hand it to `atari_ref(trunk_cache=...)`.
    Built under the `rounding` context it is meant for."""
    leaves = {k: params[k].detach().to(F64).clone().requires_grad_() for k in SECTION_PARAMS}
    return {"leaves": leaves, "flat": trunk(frames_u8, leaves, mode, wgrad, mutate),
            "key": (mode, wgrad, tuple(mutate), dict(_state))}


# mutations of the core's wiring that `atari_ref(mutate=...)` knows
CORE_MUTATIONS = ("reward_unclamped", "action_shifted", "no_bias_hh", "bias_hh_no_grad",
                  "dw_hh_unshifted", "h0_unmasked", "state_from_t_minus_2", "c0_bf16",
                  "whh_i_f_swapped")


def atari_ref(params, inputs, core_state=None, mode="a", wgrad="kernel", grads=None,
              mutate=(), trunk_fc=False, core_input=False, core_recurrent=False,
              trunk_cache=None):
    """Forward and backward of AtariNet in fp64.

    params: state_dict names -> tensors (any float dtype). inputs: state u8
    [T,B,4,84,84], reward, prev_action, done. core_state: (h0, c0) as
    [1,B,H] for the LSTM variant (recognised by `core.weight_hh_l0`, whose
    second extent is the hidden size H; 128 and 512 keep G = X + hW in fp32).
    trunk_fc, core_input, core_recurrent: the opt-in routes of the same name
    (`fused_*` in AtariNet). They move rounding points only: with every Q off
    the result does not depend on them. `core_recurrent` moves none (dW_hh is
    an fp32 sum of bf16 products on either route, cast by autograd in (a)).
    grads: {"trunk": G} backpropagates G from the flattened trunk output
    alone; {"policy_logits": Gp, "baseline": Gb} backpropagates
    (policy_logits*Gp).sum() + (baseline*Gb).sum(), plus (hT*ghT).sum() +
    (cT*gcT).sum() of the returned core state when "hT" and "cT" are given.
    Returns a dict with `trunk`, `policy_logits`, `baseline`, `hT`, `cT`,
    `dh0`, `dc0` and `grads` (name -> fp64 gradient, for every parameter that
    received one)."""
    x = inputs["state"]
    T, B = x.shape[:2]
    if trunk_cache is None:
        trunk_cache = trunk_graph(params, x.flatten(0, 1), mode, wgrad, mutate)
        retain = False
    else:
        assert trunk_cache["key"] == (mode, wgrad, tuple(m for m in mutate
                                                         if m not in CORE_MUTATIONS), dict(_state))
        retain = True
    leaves = {k: v.detach().to(F64).clone().requires_grad_() for k, v in params.items()
              if k not in SECTION_PARAMS}
    leaves.update(trunk_cache["leaves"])
    for k in SECTION_PARAMS:
        leaves[k].grad = None
    flat_full = trunk_cache["flat"]
    out = {"trunk": flat_full.detach()}
    if grads is not None and "trunk" in grads:
        flat_full.backward(grads["trunk"].to(F64), retain_graph=retain)
    else:
        flat = flat_full.detach().requires_grad_()  # the head's leaf; the trunk follows below
        top_rounds = mode == "a"
        p = {k: Q(v, "param", fwd=k not in ("core.bias_ih_l0", "core.bias_hh_l0"), bwd=top_rounds)
             for k, v in leaves.items() if k not in SECTION_PARAMS}
        h = fc_relu(flat, p["fc.weight"], p["fc.bias"], trunk_fc)
        A = p["policy.weight"].shape[0]
        reward, action = inputs["reward"].reshape(T * B), inputs["prev_action"].reshape(T * B)
        loss = 0.0
        if "core.weight_hh_l0" in p:
            w_hh = p["core.weight_hh_l0"]
            Hd = w_hh.shape[1]
            assert tuple(core_state[0].shape) == (1, B, Hd) == tuple(core_state[1].shape)
            b_ih, b_hh = p["core.bias_ih_l0"], p["core.bias_hh_l0"]
            if "no_bias_hh" in mutate:
                b_hh = b_hh * 0
            if "bias_hh_no_grad" in mutate:
                b_hh = b_hh.detach() + b_hh * 0
            Xg = core_input_proj(h, reward, action, p["core.weight_ih_l0"], b_ih, b_hh,
                                 core_input, mutate).view(T, B, -1)
            nd = (~inputs["done"].bool()).to(F64)
            if "h0_unmasked" in mutate:
                nd = nd.clone()
                nd[0] = 1.0
            h0_leaf = core_state[0].detach().to(F64).clone().requires_grad_()
            c0_leaf = core_state[1].detach().float().to(F64).clone().requires_grad_()
            h0 = Q(h0_leaf[0])  # .to(bfloat16), and its backward
            c0 = Q(c0_leaf[0]) if "c0_bf16" in mutate else c0_leaf[0]
            if "whh_i_f_swapped" in mutate:
                w_hh = torch.cat([w_hh[Hd : 2 * Hd], w_hh[:Hd], w_hh[2 * Hd :]])
            kw = {"round_g": Hd == 256, "dw_unshifted": "dw_hh_unshifted" in mutate}
            H, hT, cT = lstm(Xg, h0, c0, w_hh, nd, **kw)
            if "state_from_t_minus_2" in mutate:
                _, hT, cT = lstm(Xg[: T - 1], h0, c0, w_hh, nd[: T - 1], **kw)
            core = Q(H).flatten(0, 1)
            hT = Q(hT)  # returned as .to(core_state's fp32): its gradient is cast to bf16
            out["hT"], out["cT"] = hT.detach(), cT.detach()
            if grads is not None and "hT" in grads:
                loss = (hT * grads["hT"].to(F64)).sum() + (cT * grads["cT"].to(F64)).sum()
        else:
            onehot = torch.nn.functional.one_hot(action.long(), A).to(F64)
            core = torch.cat([h, Q(reward.reshape(-1, 1).to(F64).clamp(-1, 1)), onehot], dim=-1)
        pl = linear(core, p["policy.weight"], p["policy.bias"]).view(T, B, A)
        bl = linear(core, p["baseline.weight"], p["baseline.bias"]).view(T, B)
        out["policy_logits"], out["baseline"] = pl.detach(), bl.detach()
        if grads is not None:
            (loss + (pl * grads["policy_logits"].to(F64)).sum()
             + (bl * grads["baseline"].to(F64)).sum()).backward()
            flat_full.backward(flat.grad, retain_graph=retain)
            if "core.weight_hh_l0" in p:
                out["dh0"], out["dc0"] = h0_leaf.grad[0], c0_leaf.grad[0]
    out["grads"] = {k: v.grad.clone() for k, v in leaves.items() if v.grad is not None}
    return out


def exact(params, inputs, core_state=None, grads=None, mutate=(), **kw):
    """R_exact: every Q off. Route flags (`kw`) are accepted and change nothing."""
    with rounding(False, False):
        return atari_ref(params, inputs, core_state, "a", "kernel", grads, mutate, **kw)


# ------------------------------------------------------------------ inputs

CONV_SHAPES = {}
for _s, (_cin, _ch) in enumerate(zip((4,) + CHANS[:-1], CHANS)):
    CONV_SHAPES["sections.%d.conv" % _s] = (_ch, _cin)
    for _m in ("res0.conv0", "res0.conv1", "res1.conv0", "res1.conv1"):
        CONV_SHAPES["sections.%d.%s" % (_s, _m)] = (_ch, _ch)

# the fixed seed and tap counts of the integer-exact case; the CPU premise
# test (TestIntegerPremise) is what says that they fit
INT_SEED = 0
INT_TAPS = {"conv": 2, "conv0": 2, "conv1": 1}


def integer_case(seed=INT_SEED, taps=INT_TAPS, n_frames=3):
    """Section parameters, frames and output gradient of the integer-exact
    trunk case. Weights in {-1,0,1}: `taps` non-zero taps per output channel
    at a random position and sign; the input channel of output channel k is
    perm[k] mod C for a random permutation, so every input channel feeds the
    same number of output channels and the dgrad fan-out stays bounded.
    Biases in -1..1, frames in {0,255}, G in -1..1."""
    g = torch.Generator().manual_seed(seed)
    params = {}
    for name, (K, C) in CONV_SHAPES.items():
        w = torch.zeros(K, C, 3, 3, dtype=F64)
        for _ in range(taps[name.rsplit(".", 1)[1]]):
            perm = torch.randperm(K, generator=g)
            tap = torch.randint(0, 9, (K,), generator=g)
            sign = torch.randint(0, 2, (K,), generator=g).double() * 2 - 1
            w[torch.arange(K), perm % C, tap // 3, tap % 3] = sign
        params[name + ".weight"] = w
        params[name + ".bias"] = R.int_tensor(g, (K,), -1, 1)
    frames = torch.randint(0, 2, (n_frames, 1, 4, 84, 84), generator=g).to(torch.uint8) * 255
    G = R.int_tensor(g, (n_frames, 3872), -1, 1)
    return params, frames, G


def float_case(use_lstm, seed=0, T=3, B=2, A=6):
    """Whole-network float case: every parameter bf16-representable (so every
    mode and both references start from the same numbers), random u8 frames,
    one `done` in the middle, fixed float output gradients."""
    from moolib_amd.models.atari import AtariNet

    torch.manual_seed(100 + seed + int(use_lstm))
    model = AtariNet(num_actions=A, use_lstm=use_lstm)
    g = torch.Generator().manual_seed(200 + seed)
    params = {}
    for k, v in model.state_dict().items():
        v = v.double()
        if k.endswith("bias"):  # default conv / linear biases are tiny: give them weight
            v = torch.randn(v.shape, generator=g, dtype=F64) * 0.1
        params[k] = R.bf16_round(v)
    done = torch.zeros(T, B, dtype=torch.bool)
    done[T // 2, 0] = True
    inputs = {
        "state": torch.randint(0, 256, (T, B, 4, 84, 84), dtype=torch.uint8, generator=g),
        "reward": torch.randn(T, B, generator=g) * 2,
        "prev_action": torch.randint(0, A, (T, B), generator=g),
        "done": done,
    }
    core = None
    if use_lstm:
        core = (R.bf16_round(torch.randn(1, B, 256, generator=g, dtype=F64) * 0.3).float(),
                (torch.randn(1, B, 256, generator=g) * 0.3))
    grads = {"policy_logits": torch.randn(T, B, A, generator=g),
             "baseline": torch.randn(T, B, generator=g)}
    return params, inputs, core, grads


# the hidden unit of the never-done row whose cell state is built to cancel
CORE_PROBE_UNIT = 5
CORE_PROBE_C0 = 3.0078125  # halfway between the bf16 neighbours 3.0 and 3.015625


def core_float_case(lstm_size, A=6, T=3, B=3, seed=0):
    """Float case for the LSTM core and its routes, built like `float_case`
    (bf16-representable parameters, biases of scale 0.1, random u8 frames).
    Frames, section parameters and `fc` are the same for every `lstm_size`.

    * initial state: h0 bf16-representable, c0 fp32, both of scale 0.3;
    * done: row 0 at t=0 only (the initial state must be masked away), row 1
      at t=1, row 2 never;
    * reward: exactly +1 and -1, one value above 1, one below -1 and, in the
      never-done row, one inside (-1, 1) that bf16 does not hold;
    * prev_action: 0 and A-1 occur;
    * output gradients for policy_logits, baseline and the returned hT, cT.

    One hidden unit (CORE_PROBE_UNIT) is what lets a comparison against
    max|cT| see a single bf16 rounding of c0, which moves an element by at most
    2^-9 of itself while the bound grants 2^-8 of the tensor's maximum: cT has
    to be small where c0 is large. The unit's forget and cell biases are +6
    and -6 (ih + hh), its input bias -6 and its input weight on the reward
    column 48, so it loses 1 per step where the reward is 1/3 or more and
    stays put (0.0025 per step) where the reward is <= 0. Row 2 alone has
    positive rewards, and there c0 is 3 + 2^-7, a bf16 rounding tie: cT is
    about 2^-7, and rounding c0 moves it by 2^-7."""
    from moolib_amd.models.atari import AtariNet

    assert T == 3 and B == 3 and A >= 3
    torch.manual_seed(300 + seed)  # sections and fc are drawn before the core: shared by all widths
    model = AtariNet(num_actions=A, use_lstm=True, lstm_size=lstm_size)
    g = torch.Generator().manual_seed(400 + seed)
    params = {}
    for k, v in model.state_dict().items():
        v = v.double()
        if k.endswith("bias") or ".bias_" in k:
            v = torch.randn(v.shape, generator=g, dtype=F64) * 0.1
        params[k] = R.bf16_round(v)
    u, Hd = CORE_PROBE_UNIT, lstm_size
    for k in ("core.bias_ih_l0", "core.bias_hh_l0"):
        params[k][u], params[k][Hd + u], params[k][2 * Hd + u] = -3.0, 3.0, -3.0
    params["core.weight_ih_l0"][u, model.fc.out_features] = 48.0
    g = torch.Generator().manual_seed(500 + seed)  # inputs: the same for every width
    done = torch.zeros(T, B, dtype=torch.bool)
    done[0, 0] = True
    done[1, 1] = True
    inputs = {
        "state": torch.randint(0, 256, (T, B, 4, 84, 84), dtype=torch.uint8, generator=g),
        "reward": torch.tensor([[-1.0, -0.71, 0.3337], [-2.25, 0.0, 1.0], [0.0, -0.125, 2.5]]),
        "prev_action": torch.tensor([[0, A - 1, 2], [1, 0, A - 1], [2, 1, 0]]),
        "done": done,
    }
    grads = {"policy_logits": torch.randn(T, B, A, generator=g),
             "baseline": torch.randn(T, B, generator=g)}
    g = torch.Generator().manual_seed(600 + seed + lstm_size)
    h0 = R.bf16_round(torch.randn(1, B, Hd, generator=g, dtype=F64) * 0.3).float()
    c0 = torch.randn(1, B, Hd, generator=g) * 0.3
    c0[0, 2, u] = CORE_PROBE_C0
    grads["hT"] = torch.randn(B, Hd, generator=g)
    grads["cT"] = torch.randn(B, Hd, generator=g)
    return params, inputs, (h0, c0), grads


# ------------------------------------------------------------------ comparisons


def bit_equal(got, ref, dtype):
    """The integer-exact comparison: `got` (a tensor of `dtype` from the GPU
    path) against the fp64 reference cast to that dtype."""
    return got.dtype == dtype and got.shape == ref.shape and torch.equal(got, ref.to(dtype))


def wrw_within(got, ref_exact):
    """MIOpen wrw leg: one bf16 rounding of the exact value, per element."""
    return bool(((got.double() - ref_exact).abs() <= R.BF16_STEP * ref_exact.abs()).all())


def float_bound(exact_t, emul_t):
    """(d, bound): d = max|R_emul - R_exact|, bound = 2 d + 2^-8 max|R_exact|."""
    d = (emul_t - exact_t).abs().max().item()
    return d, 2 * d + R.BF16_STEP * exact_t.abs().max().item()


def float_within(got, exact_t, bound):
    return got.shape == exact_t.shape and (got.double() - exact_t).abs().max().item() <= bound
