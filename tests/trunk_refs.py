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
    def forward(ctx, X, h0, c0, w, nd, rounding_on):
        z = torch.zeros
        d = {"X": X, "h0": h0, "c0": c0, "w": w, "nd": nd,
             "gH": z(X.shape[0], X.shape[1], h0.shape[1], dtype=F64),
             "ghT": z(h0.shape, dtype=F64), "gcT": z(h0.shape, dtype=F64)}
        out = R.lstm_emul(d, rounding_on)
        ctx.d, ctx.rounding_on = d, rounding_on
        return out["H"], out["hT"], out["cT"]

    @staticmethod
    def backward(ctx, gH, ghT, gcT):
        out = R.lstm_emul(dict(ctx.d, gH=gH, ghT=ghT, gcT=gcT), ctx.rounding_on)
        return out["dX"], out["dh0"], out["dc0"], out["dW"], None, None


def lstm(X, h0, c0, w, nd, force_emul=False):
    """lstm_emul when the activation Qs are on, else the plain recurrence;
    `force_emul` runs lstm_emul with its rounding off instead (the two must
    then agree)."""
    if _state["act"] or force_emul:
        return _LstmEmulFn.apply(X, h0, c0, w, nd, _state["act"])
    return lstm_plain(X, h0, c0, w, nd)


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


def atari_ref(params, inputs, core_state=None, mode="a", wgrad="kernel", grads=None,
              mutate=()):
    """Forward and backward of AtariNet in fp64.

    params: state_dict names -> tensors (any float dtype). inputs: state u8
    [T,B,4,84,84], reward, prev_action, done. core_state: (h0, c0) as
    [1,B,256] for the LSTM variant (recognised by `core.weight_hh_l0`).
    grads: {"trunk": G} backpropagates G from the flattened trunk output
    alone; {"policy_logits": Gp, "baseline": Gb} backpropagates
    (policy_logits*Gp).sum() + (baseline*Gb).sum(). Returns a dict with
    `trunk`, `policy_logits`, `baseline`, `hT`, `cT` and `grads` (name -> fp64
    gradient, for every parameter that received one)."""
    leaves = {k: v.detach().to(F64).clone().requires_grad_() for k, v in params.items()}
    x = inputs["state"]
    T, B = x.shape[:2]
    flat = trunk(x.flatten(0, 1), {k: leaves[k] for k in SECTION_PARAMS}, mode, wgrad, mutate)
    out = {"trunk": flat.detach()}
    if grads is not None and "trunk" in grads:
        flat.backward(grads["trunk"].to(F64))
    else:
        top_rounds = mode == "a"
        p = {k: Q(v, "param", fwd=k not in ("core.bias_ih_l0", "core.bias_hh_l0"), bwd=top_rounds)
             for k, v in leaves.items() if k not in SECTION_PARAMS}
        h = torch.relu(linear(flat, p["fc.weight"], p["fc.bias"]))
        A = p["policy.weight"].shape[0]
        onehot = torch.nn.functional.one_hot(inputs["prev_action"].reshape(T * B).long(), A)
        reward = Q(inputs["reward"].reshape(T * B, 1).to(F64).clamp(-1, 1))
        core = torch.cat([h, reward, onehot.to(F64)], dim=-1)
        if "core.weight_hh_l0" in p:
            # bias_ih + bias_hh is formed in the parameters' dtype, then bf16
            Xg = linear(core, p["core.weight_ih_l0"], p["core.bias_ih_l0"] + p["core.bias_hh_l0"])
            nd = (~inputs["done"].bool()).to(F64)
            h0 = Q(core_state[0][0].to(F64))
            c0 = core_state[1][0].float().to(F64)
            H, hT, cT = lstm(Xg.view(T, B, -1), h0, c0, p["core.weight_hh_l0"], nd)
            core = Q(H).flatten(0, 1)
            out["hT"], out["cT"] = hT.detach(), cT.detach()
        pl = linear(core, p["policy.weight"], p["policy.bias"]).view(T, B, A)
        bl = linear(core, p["baseline.weight"], p["baseline.bias"]).view(T, B)
        out["policy_logits"], out["baseline"] = pl.detach(), bl.detach()
        if grads is not None:
            ((pl * grads["policy_logits"].to(F64)).sum()
             + (bl * grads["baseline"].to(F64)).sum()).backward()
    out["grads"] = {k: v.grad for k, v in leaves.items() if v.grad is not None}
    return out


def exact(params, inputs, core_state=None, grads=None, mutate=()):
    """R_exact: every Q off."""
    with rounding(False, False):
        return atari_ref(params, inputs, core_state, "a", "kernel", grads, mutate)


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
