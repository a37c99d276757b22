"""Plain fp64 CPU references for the HIP kernels, plus the input generators
the edge-shape tests use (tests/test_kernel_edges.py; docs/KERNEL_TESTS.md).

Everything here runs on the CPU in float64 and is written as the textbook
definition of the op (tap loops, explicit recurrences), NOT by calling the
torch op it stands in for: the CPU self-checks in test_kernel_edges.py
compare these against torch's own fp64 ops, so a reference and a kernel
cannot share a mistake unnoticed.

Integer-exactness: the linear kernels accumulate in fp32. With small-integer
inputs every product and partial sum is an integer far below 2**24, so fp32
accumulation is exact in any order (MFMA, LDS and global float atomics
included) and the kernel must equal the fp64 reference cast to the output
dtype bit for bit.
"""
import numpy as np
import torch

BF16_STEP = 2.0 ** -8  # one bf16 rounding step (8 significand bits), relative
F32_EPS = 2.0 ** -24   # fp32 unit roundoff


def bf16_round(t):
    """Round to bf16 (nearest even) and come back to float64."""
    return t.to(torch.bfloat16).to(torch.float64)


def int_tensor(gen, shape, lo, hi):
    """float64 tensor of integers drawn uniformly from lo..hi inclusive."""
    return torch.randint(lo, hi + 1, shape, generator=gen).to(torch.float64)


def assert_int_exact(*tensors, limit=2 ** 24):
    """Every value is an integer below `limit` in magnitude, i.e. exactly
    representable (and exactly accumulated) in fp32."""
    for t in tensors:
        assert torch.equal(t, t.round()), "non-integer reference value"
        assert t.abs().max().item() < limit, t.abs().max().item()


# ------------------------------------------------------------------ conv3x3


def _pad1(x):
    N, C, H, W = x.shape
    xp = x.new_zeros(N, C, H + 2, W + 2)
    xp[:, :, 1 : H + 1, 1 : W + 1] = x
    return xp


def conv3x3_ref(x, w):
    """3x3 / stride 1 / pad 1 cross-correlation, x [N,C,H,W], w [K,C,3,3]."""
    N, C, H, W = x.shape
    xp = _pad1(x.double())
    w = w.double()
    y = x.new_zeros(N, w.shape[0], H, W, dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            y += torch.einsum("nchw,kc->nkhw", xp[:, :, kh : kh + H, kw : kw + W], w[:, :, kh, kw])
    return y


def conv3x3_abs_ref(x, w):
    """sum |x||w| over the taps: the scale of the fp32 accumulation error."""
    return conv3x3_ref(x.double().abs(), w.double().abs())


def conv3x3_fused_ref(x, w, relu_in=False, bias_in=None, epi=0, bias1=None, res=None,
                      bias2=None, return_scale=False):
    """The fused kernel's op in fp64. Inputs hold bf16-representable values.
    The prologue relu(x + bias_in) is rounded to bf16 as the kernel rounds it
    (fp32 add, then bf16); the rest is exact. Returns the fp64 result BEFORE
    the output cast; with return_scale also sum|terms| for error bounds."""
    xd = x.double()
    if relu_in:
        if bias_in is not None:
            xd = (x.float() + bias_in.float().view(1, -1, 1, 1)).double()
        xd = bf16_round(torch.relu(xd))
    y = conv3x3_ref(xd, w)
    scale = conv3x3_abs_ref(xd, w)
    v = lambda b: b.double().view(1, -1, 1, 1)
    if epi in (1, 2, 3):
        y = y + v(bias1)
        scale = scale + v(bias1).abs()
    if epi == 2:
        y = torch.relu(y)
    if epi == 3:
        y = y + res.double()
        scale = scale + res.double().abs()
        if bias2 is not None:
            y = y + v(bias2)
            scale = scale + v(bias2).abs()
    return (y, scale) if return_scale else y


def conv3x3_dgrad_ref(dy, w):
    """Input gradient of conv3x3_ref: dx[n,c,h,w] = sum dy[n,k,h-kh+1,w-kw+1] w[k,c,kh,kw]."""
    N, K, H, W = dy.shape
    dyp = _pad1(dy.double())
    w = w.double()
    dx = dy.new_zeros(N, w.shape[1], H, W, dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            # output pixel (h - kh + 1, w - kw + 1) -> padded index (h + 2 - kh, w + 2 - kw)
            win = dyp[:, :, 2 - kh : 2 - kh + H, 2 - kw : 2 - kw + W]
            dx += torch.einsum("nkhw,kc->nchw", win, w[:, :, kh, kw])
    return dx


def conv3x3_wgrad_ref(x, dy):
    """Weight gradient of conv3x3_ref: dw[k,c,kh,kw] = sum dy[n,k,h,w] xpad[n,c,h+kh,w+kw]."""
    N, C, H, W = x.shape
    xp = _pad1(x.double())
    dy = dy.double()
    dw = x.new_zeros(dy.shape[1], C, 3, 3, dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            dw[:, :, kh, kw] = torch.einsum("nkhw,nchw->kc", dy, xp[:, :, kh : kh + H, kw : kw + W])
    return dw


# ------------------------------------------------------- maxpool 3x3 / s2 / p1


def maxpool3x3s2_ref(x, gout=None):
    """Explicit-loop max_pool2d(x, 3, stride=2, padding=1) in fp64.

    The maximum is the FIRST one in row-major scan order of the window, a
    NaN wins over everything (the last NaN of the window is the one that is
    kept), and a window of all -inf selects its first in-bounds element:
    torch's CPU semantics. With `gout` also returns the input gradient."""
    x = x.double()
    N, C, H, W = x.shape
    OH, OW = (H + 1) // 2, (W + 1) // 2
    out = x.new_empty(N, C, OH, OW)
    gin = torch.zeros_like(x) if gout is not None else None
    for oh in range(OH):
        for ow in range(OW):
            best = None
            for kh in range(3):
                ih = oh * 2 - 1 + kh
                if ih < 0 or ih >= H:
                    continue
                for kw in range(3):
                    iw = ow * 2 - 1 + kw
                    if iw < 0 or iw >= W:
                        continue
                    v = x[:, :, ih, iw]
                    if best is None:
                        best = v.clone()
                        bih = torch.full((N, C), ih)
                        biw = torch.full((N, C), iw)
                        continue
                    take = (v > best) | torch.isnan(v)
                    best = torch.where(take, v, best)
                    bih = torch.where(take, torch.full_like(bih, ih), bih)
                    biw = torch.where(take, torch.full_like(biw, iw), biw)
            out[:, :, oh, ow] = best
            if gin is not None:
                n_i, c_i = torch.meshgrid(torch.arange(N), torch.arange(C), indexing="ij")
                gin.index_put_((n_i, c_i, bih, biw), gout.double()[:, :, oh, ow], accumulate=True)
    return out if gout is None else (out, gin)


def maxpool_tie_fraction(x):
    """Fraction of pooling windows whose maximum is attained more than once."""
    x = x.double()
    N, C, H, W = x.shape
    OH, OW = (H + 1) // 2, (W + 1) // 2
    tied = 0
    for oh in range(OH):
        for ow in range(OW):
            win = x[:, :, max(oh * 2 - 1, 0) : oh * 2 + 2, max(ow * 2 - 1, 0) : ow * 2 + 2]
            flat = win.reshape(N, C, -1)
            tied += ((flat == flat.amax(-1, keepdim=True)).sum(-1) > 1).sum().item()
    return tied / (N * C * OH * OW)


# ------------------------------------------------------- channel-sum mapping


def channel_sum_blocks(total8, c8n, threads=256, cap=None):
    """Grid size of bias_relu_bwd / channel_sum_fp32 (channelSumBlocks in
    hip/kernels.hip): the cap, then rounded down to a multiple of the odd
    part of c8n whenever the grid-stride loop iterates."""
    if cap is None:
        cap = min(max(total8 // 3000, 256), 768)
    blocks = min((total8 + threads - 1) // threads, cap)
    odd = c8n
    while odd % 2 == 0:
        odd //= 2
    if blocks * threads < total8:
        blocks = max(blocks // odd, 1) * odd
    return blocks


def channel_sum_blocks_unrounded(total8, c8n, threads=256):
    """The grid the kernels were launched with before the rounding fix."""
    return min((total8 + threads - 1) // threads, min(max(total8 // 3000, 256), 768))


def channel_sum_miscredited(total8, c8n, blocks, threads=256):
    """Model of the kernels' thread -> channel-octet mapping: octet `tid`
    belongs to channel group tid % c8n, and is credited to the group of the
    thread that visits it, tid0 % c8n with tid0 = tid % (threads*blocks).
    Returns how many octets land in the wrong group."""
    tid = np.arange(total8, dtype=np.int64)
    stride = threads * blocks
    return int(((tid % stride) % c8n != tid % c8n).sum())


# ------------------------------------------------------------------- conv1


def conv1_u8_ref(x_u8, w, b, scale):
    """uint8 frames * scale -> conv3x3 + bias, fp64. w [16,4,3,3] and b hold
    bf16-representable values; `scale` is used as the fp32 value the kernel
    receives. Returns (ref, S) with S = sum|x*scale||w| + |b|."""
    s = float(np.float32(scale))
    xs = x_u8.double() * s
    y = conv3x3_ref(xs, w) + b.double().view(1, -1, 1, 1)
    S = conv3x3_abs_ref(xs, w) + b.double().abs().view(1, -1, 1, 1)
    return y, S


# -------------------------------------------------------------------- losses


def impala_loss_ref(logits, actions, pg_adv, vs, baseline, entropy_cost, baseline_cost,
                    dtype=torch.float64, grad_scale=1.0):
    """The three IMPALA loss parts and d(grad_scale*total)/d(logits, baseline)
    from their definitions, in `dtype`. Returns (parts[3], glogits, gbaseline)."""
    lg = logits.detach().to(dtype).clone().requires_grad_()
    bl = baseline.detach().to(dtype).clone().requires_grad_()
    adv, v = pg_adv.to(dtype), vs.to(dtype)
    z = lg - lg.max(-1, keepdim=True).values
    logp = z - z.exp().sum(-1, keepdim=True).log()
    chosen = logp.gather(-1, actions.long().unsqueeze(-1)).squeeze(-1)
    pg = (-chosen * adv).mean()
    bloss = baseline_cost * 0.5 * ((v - bl) ** 2).mean()
    ent = entropy_cost * (logp.exp() * logp).sum(-1).mean()  # -mean(H) * cost
    (grad_scale * (pg + bloss + ent)).backward()
    return torch.stack([pg, bloss, ent]).detach(), lg.grad, bl.grad


def impala_pg_abs(logits, actions, pg_adv):
    """mean |log pi(a) * adv|: the magnitude of the terms the policy-gradient
    loss sums (they cancel, so the loss itself can be much smaller)."""
    logp = torch.log_softmax(logits.double(), dim=-1)
    chosen = logp.gather(-1, actions.long().unsqueeze(-1)).squeeze(-1)
    return (chosen * pg_adv.double()).abs().mean().item()


def impala_loss_eager(logits, actions, pg_adv, vs, baseline, entropy_cost, baseline_cost):
    """The project's eager fp32 path (ops/losses.py) on the CPU, same outputs."""
    from moolib_amd.ops import losses

    lg = logits.detach().float().clone().requires_grad_()
    bl = baseline.detach().float().clone().requires_grad_()
    pg = losses.policy_gradient_loss(lg, actions, pg_adv.float())
    bloss = baseline_cost * losses.baseline_loss(vs.float() - bl)
    ent = entropy_cost * losses.entropy_loss(lg)
    (pg + bloss + ent).backward()
    return torch.stack([pg, bloss, ent]).detach(), lg.grad, bl.grad


def vtrace_ref(log_rhos, discounts, rewards, values, bootstrap, clip_rho, clip_pg_rho,
               dtype=torch.float64):
    """V-trace recursion written out per time step, in `dtype`."""
    lr, g, r, v, bs = (t.to(dtype) for t in (log_rhos, discounts, rewards, values, bootstrap))
    T = lr.shape[0]
    rho = lr.exp()
    crho = rho if clip_rho is None else rho.clamp(max=clip_rho)
    pgrho = rho if clip_pg_rho is None else rho.clamp(max=clip_pg_rho)
    c = rho.clamp(max=1.0)
    vs = torch.empty_like(v)
    acc = torch.zeros_like(bs)
    for t in reversed(range(T)):
        nxt = bs if t == T - 1 else v[t + 1]
        acc = crho[t] * (r[t] + g[t] * nxt - v[t]) + g[t] * c[t] * acc
        vs[t] = acc + v[t]
    pg = torch.empty_like(v)
    for t in range(T):
        nxt = bs if t == T - 1 else vs[t + 1]
        pg[t] = pgrho[t] * (r[t] + g[t] * nxt - v[t])
    return vs, pg


# ---------------------------------------------------------------------- LSTM


def lstm_inputs(gen, T, B, hidden=256):
    """bf16-representable fp64 inputs and output gradients for one masked
    LSTM scan. Mask rows (when B allows): row 0 is done at t=0 only, row 1 is
    done at every step, row 2 is never done; the rest are random."""
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    d = {
        "X": bf16_round(rn(T, B, 4 * hidden) * 0.5),
        "h0": bf16_round(rn(B, hidden) * 0.3),
        "c0": (rn(B, hidden) * 0.3).float().double(),
        "w": bf16_round(rn(4 * hidden, hidden) * 0.05),
        "gH": bf16_round(rn(T, B, hidden)),
        "ghT": bf16_round(rn(B, hidden)),
        "gcT": rn(B, hidden).float().double(),
    }
    nd = (torch.rand(T, B, generator=gen) > 0.2).double()
    nd[0, 0] = 0.0
    nd[1:, 0] = 1.0
    if B > 1:
        nd[:, 1] = 0.0
    if B > 2:
        nd[:, 2] = 1.0
    d["nd"] = nd
    return d


def lstm_exact(d):
    """R_exact: the plain masked recurrence in fp64, gradients by autograd of
    loss = (H*gH).sum() + (hT*ghT).sum() + (cT*gcT).sum()."""
    X, h0, c0, w = (d[k].clone().requires_grad_() for k in ("X", "h0", "c0", "w"))
    nd = d["nd"]
    h, c = h0, c0
    Hs = []
    for t in range(X.shape[0]):
        m = nd[t].unsqueeze(-1)
        h, c = h * m, c * m
        i, f, g, o = (X[t] + h @ w.t()).chunk(4, dim=-1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        Hs.append(h)
    H = torch.stack(Hs)
    ((H * d["gH"]).sum() + (h * d["ghT"]).sum() + (c * d["gcT"]).sum()).backward()
    return {"H": H.detach(), "hT": h.detach(), "cT": c.detach(), "dX": X.grad, "dh0": h0.grad,
            "dc0": c0.grad, "dW": w.grad}


def lstm_emul(d, rounding=True):
    """R_emul: the same recurrence and its hand-written backward in fp64 with
    the kernel's bf16 rounding points (hip/lstm.hip.inc, ops/lstm.py):
    h after masking and after each step, G = X + hW before the gates, the
    saved gates, dG before the dG.W GEMM and in dW, and dh0.
    rounding=False switches every rounding point off."""
    r = bf16_round if rounding else (lambda t: t)
    X, h0, c0, w, nd = d["X"], d["h0"], d["c0"], d["w"], d["nd"]
    T, B, _ = X.shape
    h, c = h0, c0
    H, gates, cs, hm = [], [], [], []
    for t in range(T):
        m = nd[t].unsqueeze(-1)
        h, c = r(h * m), c * m
        hm.append(h)
        G = r(X[t] + h @ w.t())
        i, f, g, o = G.chunk(4, dim=-1)
        i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
        c = f * c + i * g
        h = r(o * torch.tanh(c))
        H.append(h)
        cs.append(c)
        gates.append(tuple(r(a) for a in (i, f, g, o)))
    out = {"H": torch.stack(H), "hT": h, "cT": c}

    dh, dc = d["ghT"].clone(), d["gcT"].clone()
    dX = torch.empty_like(X)
    dW = torch.zeros_like(w)
    for t in reversed(range(T)):
        m = nd[t].unsqueeze(-1)
        gi, gf, gg, go = gates[t]
        cm = m * (c0 if t == 0 else cs[t - 1])
        dht = dh + d["gH"][t]
        tc = torch.tanh(cs[t])
        dcn = dc + dht * go * (1 - tc * tc)
        dG = r(torch.cat([
            dcn * gg * gi * (1 - gi),
            dcn * cm * gf * (1 - gf),
            dcn * gi * (1 - gg * gg),
            dht * tc * go * (1 - go),
        ], dim=-1))
        dX[t] = dG
        dW += dG.t() @ hm[t]
        dc = m * gf * dcn
        dh = m * (dG @ w)
    out.update({"dX": dX, "dh0": r(dh), "dc0": dc, "dW": dW})
    return out


LSTM_TENSORS = ("H", "hT", "cT", "dX", "dh0", "dc0", "dW")


def lstm_bounds(exact, emul):
    """Per tensor: d = max|R_emul - R_exact| and the test bound
    2*d + 2**-8 * max|R_exact| (see docs/KERNEL_TESTS.md)."""
    out = {}
    for k in LSTM_TENSORS:
        dd = (emul[k] - exact[k]).abs().max().item()
        out[k] = (dd, 2 * dd + BF16_STEP * exact[k].abs().max().item())
    return out


def fp32_accum_bound(n_terms, S):
    """|fp32 accumulation of n terms - exact| <= n * 2**-24 * sum|terms|
    (first-order; callers add their own slack factor)."""
    return n_terms * F32_EPS * S
