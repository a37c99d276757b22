"""Fused masked-LSTM sequence scan (gfx950 MFMA kernel dispatch).

Replaces the T-step Python loop over nn.LSTM in the IMPALA model with one
kernel launch per direction (see hip/lstm.hip.inc). The input projection
x @ W_ih^T + b runs as one hipBLASLt GEMM over all T steps; the recurrent
part (h @ W_hh^T on mfma_f32_16x16x32_bf16, gates, done-masking) runs in
one launch per direction, on one of two kernel families:

* hidden size 256 (the IMPALA config): hip/lstm.hip.inc, with h, c and the
  pre-activation gates resident in LDS. Always saves gates and cell states.
* hidden sizes 128 and 512 (512 is R2D2's core): hip/lstm_wide.hip.inc, with
  c, the gates and the running gradients in registers and only the MFMA A
  operand in LDS. When grad mode is off, or no input requires a gradient, its
  forward-only variant runs: the same instruction sequence without the
  [T,B,4H] gate and [T,B,H] cell-state stores, bit-identical H, hT and cT.

Any other hidden size is not served here (`available` is False).
notdone is 0 or 1; the kernels do not check it.

`core_input_projection` is the front end of the same core as one op
(hip/lstm_input.hip.inc): X = feat @ W_ih[:, :256]^T + the clamped reward times
its column + the previous action's column + both biases, from weight_ih_l0 as
nn.LSTM stores it. It replaces one_hot, clamp, cat, the bias add, the weight
cast and an odd-K GEMM, forward and backward.

`fused_lstm_scan(..., native_whh=True)` puts what is left around weight_hh_l0
on kernels too (hip/lstm_whh.hip.inc): `pack_whh` writes both packed layouts
of the weight in one launch, and `recurrent_weight_grad` is the backward's
dW_hh = dG^T @ (shifted, masked H) without the copy of H, the mask multiply,
the fp32 casts and the fp32 GEMM.
"""
import os

import torch
import torch.nn.functional as F


WIDE_SIZES = (128, 512)  # served by hip/lstm_wide.hip.inc; 256 by hip/lstm.hip.inc
# core_input_projection on the GPU: the feature width and the widest action set
# (_kernels.LSTM_INPUT_MAX_ACTIONS is the same number: the reward column, the
# action columns and the bias column of the weight-gradient product fill 64)
CORE_INPUT_FEATURES = 256
CORE_INPUT_MAX_ACTIONS = 62


def _kernels():
    try:
        from moolib_amd import _kernels as k

        return k
    except ImportError:
        return None


def available(hidden_size, device):
    return (
        hidden_size in (256,) + WIDE_SIZES
        and device.type == "cuda"
        and _kernels() is not None
        and not os.environ.get("MOOLIB_AMD_NO_LSTM_KERNEL")
    )


def pack_mfma_b(w):
    """Pack W [K, N] into per-lane mfma_f32_16x16x32_bf16 B-fragment order:
    fragment (ct, kk), lane l = hi*16+lo, elem e -> W[kk*32+hi*8+e][ct*16+lo],
    laid out so each lane loads its 8 bf16 with one 16-byte read."""
    K, N = w.shape
    v = w.view(K // 32, 4, 8, N // 16, 16)  # [kk, hi, e, ct, lo]
    return v.permute(3, 0, 1, 4, 2).contiguous().view(-1)


class _FusedLSTMScan(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, notdone, h0, c0, w_hh):
        k = _kernels()
        w = w_hh.detach().to(torch.bfloat16)
        packed_t = pack_mfma_b(w.t().contiguous())  # [H, 4H]: K=256, N=1024
        # the kernels take contiguous operands only; the backward reuses these
        notdone, h0, c0 = notdone.contiguous(), h0.contiguous(), c0.contiguous()
        H, gates, cs, hT, cT = k.lstm_fused_fwd(X.contiguous(), notdone, h0, c0, packed_t)
        ctx.save_for_backward(gates, cs, c0, notdone, w, h0, H)
        return H, hT, cT

    @staticmethod
    def backward(ctx, dH, dhT, dcT):
        k = _kernels()
        gates, cs, c0, notdone, w, h0, H = ctx.saved_tensors
        packed_n = pack_mfma_b(w.contiguous())  # [4H, H]: K=1024, N=256
        empty = torch.Tensor()
        dG, dh0, dc0 = k.lstm_fused_bwd(
            gates,
            cs,
            c0,
            notdone,
            dH.contiguous().to(torch.bfloat16),
            dhT.contiguous().to(torch.bfloat16) if dhT is not None else empty,
            dcT.contiguous().float() if dcT is not None else empty,
            packed_n,
        )
        T, B, _ = dG.shape
        # dW_hh = dG^T @ h_masked_prev  (h_masked[t] = nd[t] * H[t-1], H[-1]=h0)
        Hm = torch.cat([h0.unsqueeze(0), H[:-1]]) * notdone.unsqueeze(-1).to(H.dtype)
        dW = dG.reshape(T * B, -1).t().float() @ Hm.reshape(T * B, -1).float()
        return dG, None, dh0, dc0, dW

    # note: returned grads match input dtypes: X bf16 <- dG bf16; h0 bf16 <- dh0 bf16;
    # c0 f32 <- dc0 f32; w_hh gets fp32 (autograd casts to the param dtype).


class _WideLSTMScan(torch.autograd.Function):
    """The same contract as _FusedLSTMScan over the 128/512 kernels."""

    @staticmethod
    def forward(ctx, X, notdone, h0, c0, w_hh):
        k = _kernels()
        w = w_hh.detach().to(torch.bfloat16)
        packed_t = pack_mfma_b(w.t().contiguous())  # [H, 4H]
        notdone, h0, c0 = notdone.contiguous(), h0.contiguous(), c0.contiguous()
        H, gates, cs, hT, cT = k.lstm_wide_fwd(X.contiguous(), notdone, h0, c0, packed_t, True)
        ctx.save_for_backward(gates, cs, c0, notdone, w, h0, H)
        return H, hT, cT

    @staticmethod
    def backward(ctx, dH, dhT, dcT):
        k = _kernels()
        gates, cs, c0, notdone, w, h0, H = ctx.saved_tensors
        packed_n = pack_mfma_b(w.contiguous())  # [4H, H]
        empty = torch.Tensor()
        dG, dh0, dc0 = k.lstm_wide_bwd(
            gates,
            cs,
            c0,
            notdone,
            dH.contiguous().to(torch.bfloat16),
            dhT.contiguous().to(torch.bfloat16) if dhT is not None else empty,
            dcT.contiguous().float() if dcT is not None else empty,
            packed_n,
        )
        T, B, _ = dG.shape
        # dW_hh = dG^T @ h_masked_prev, as in _FusedLSTMScan.backward
        Hm = torch.cat([h0.unsqueeze(0), H[:-1]]) * notdone.unsqueeze(-1).to(H.dtype)
        dW = dG.reshape(T * B, -1).t().float() @ Hm.reshape(T * B, -1).float()
        return dG, None, dh0, dc0, dW


def _native_whh(t):
    return t.is_cuda and _kernels() is not None


def pack_whh(w_hh):
    """weight_hh_l0 [4H,H] -> (packed_t, packed_n): pack_mfma_b of bf16(w)^T
    (the forward scan's B operand) and of bf16(w) (the backward's), bit for
    bit. On a GPU with _kernels built, for an fp32 or bf16 weight, one launch
    that reads the weight once (H in 128/256/512, anything else raises);
    elsewhere the two pack_mfma_b calls."""
    w = w_hh.detach()
    if _native_whh(w) and w.dtype in (torch.float32, torch.bfloat16):
        return tuple(_kernels().lstm_whh_pack(w.contiguous()))
    w = w.to(torch.bfloat16)
    return pack_mfma_b(w.t().contiguous()), pack_mfma_b(w.contiguous())


def recurrent_weight_grad(dG, H, h0, notdone):
    """dW_hh [4H,H] fp32 = dG^T @ Hp over all T*B rows, with
    Hp[t] = where(notdone[t] != 0, h0 if t == 0 else H[t-1], 0).
    dG [T,B,4H], H [T,B,H], h0 [B,H], notdone [T,B].

    On a GPU with _kernels built: bf16 dG, H and h0, fp32 notdone, H in
    128/256/512 (anything else raises); Hp is formed as the operand is
    fetched, the product runs on the MFMA in fp32 and is summed in a fixed
    order, so two calls agree bit for bit. No host sync. Elsewhere the same
    in plain torch, in fp32."""
    if _native_whh(dG):
        return _kernels().lstm_whh_grad(
            dG.contiguous(), H.contiguous(), h0.contiguous(), notdone.contiguous()
        )
    T, B, _ = dG.shape
    prev = torch.cat([h0.unsqueeze(0), H[:-1]])
    Hp = torch.where(notdone.unsqueeze(-1) != 0, prev, prev.new_zeros(()))
    return dG.reshape(T * B, -1).t().float() @ Hp.reshape(T * B, -1).float()


class _NativeWhhScan(torch.autograd.Function):
    """Either kernel family's scan with weight_hh_l0 handled by pack_whh and
    recurrent_weight_grad: packed_n is saved in place of the bf16 weight."""

    @staticmethod
    def forward(ctx, X, notdone, h0, c0, w_hh):
        k = _kernels()
        packed_t, packed_n = pack_whh(w_hh)
        notdone, h0, c0 = notdone.contiguous(), h0.contiguous(), c0.contiguous()
        if w_hh.shape[1] == 256:
            H, gates, cs, hT, cT = k.lstm_fused_fwd(X.contiguous(), notdone, h0, c0, packed_t)
        else:
            H, gates, cs, hT, cT = k.lstm_wide_fwd(X.contiguous(), notdone, h0, c0, packed_t, True)
        ctx.save_for_backward(gates, cs, c0, notdone, packed_n, h0, H)
        return H, hT, cT

    @staticmethod
    def backward(ctx, dH, dhT, dcT):
        k = _kernels()
        gates, cs, c0, notdone, packed_n, h0, H = ctx.saved_tensors
        empty = torch.Tensor()
        bwd = k.lstm_fused_bwd if H.shape[2] == 256 else k.lstm_wide_bwd
        dG, dh0, dc0 = bwd(
            gates,
            cs,
            c0,
            notdone,
            dH.contiguous().to(torch.bfloat16),
            dhT.contiguous().to(torch.bfloat16) if dhT is not None else empty,
            dcT.contiguous().float() if dcT is not None else empty,
            packed_n,
        )
        return dG, None, dh0, dc0, recurrent_weight_grad(dG, H, h0, notdone)


def fused_lstm_scan(X, notdone, h0, c0, w_hh, native_whh=False):
    """X [T,B,4H] bf16; notdone [T,B] f32, 0 or 1; h0 [B,H] bf16; c0 [B,H] f32;
    w_hh [4H,H], with H in (128, 256, 512).
    Returns (H [T,B,H] bf16, hT [B,H] bf16, cT [B,H] f32).

    H == 256 runs the LDS-resident kernels. 128 and 512 run the register-
    resident ones, forward-only (nothing saved, plain tensors returned) when
    grad mode is off or no input requires a gradient.

    native_whh=True keeps the same scan kernels and moves everything else that
    touches w_hh onto hip/lstm_whh.hip.inc: one pack launch in the forward
    (its second output saved for the backward) and recurrent_weight_grad for
    dW. All outputs and gradients but dW are bit-identical to the default; dW
    differs by fp32 summation order only."""
    hidden = w_hh.shape[1]
    if hidden != 256 and hidden not in WIDE_SIZES:
        raise ValueError(
            "fused_lstm_scan: hidden size %d has no kernel (128, 256 and 512 do)" % hidden
        )
    wants_grad = torch.is_grad_enabled() and any(t.requires_grad for t in (X, h0, c0, w_hh))
    if native_whh and (hidden == 256 or wants_grad):
        return _NativeWhhScan.apply(X, notdone, h0, c0, w_hh)
    if hidden == 256:
        return _FusedLSTMScan.apply(X, notdone, h0, c0, w_hh)
    if wants_grad:
        return _WideLSTMScan.apply(X, notdone, h0, c0, w_hh)
    if native_whh:
        packed_t = pack_whh(w_hh)[0]
    else:
        packed_t = pack_mfma_b(w_hh.detach().to(torch.bfloat16).t().contiguous())
    H, hT, cT = _kernels().lstm_wide_fwd(
        X.contiguous(), notdone.contiguous(), h0.contiguous(), c0.contiguous(), packed_t, False
    )
    return H, hT, cT


def core_input_available(feat_width, num_actions, hidden_size, device):
    """Whether core_input_projection runs its kernels for this shape on `device`."""
    return (
        feat_width == CORE_INPUT_FEATURES
        and 1 <= num_actions <= CORE_INPUT_MAX_ACTIONS
        and hidden_size in (256,) + WIDE_SIZES
        and device.type == "cuda"
        and _kernels() is not None
    )


def core_input_eager(feat, reward, prev_action, weight_ih, bias_ih, bias_hh):
    """The projection in plain torch, in feat's dtype: what the kernels compute,
    as AtariNet wrote it before them (one_hot, clamp, cat, F.linear). An action
    outside [0, A) gives an all-zero one-hot row."""
    A = weight_ih.shape[1] - feat.shape[1] - 1
    action = prev_action.reshape(-1).to(torch.int64)
    valid = ((action >= 0) & (action < A)).unsqueeze(-1)
    onehot = F.one_hot(action.clamp(0, A - 1), A).to(feat.dtype) * valid.to(feat.dtype)
    clipped = reward.reshape(-1, 1).clamp(-1, 1).to(feat.dtype)
    x = torch.cat([feat, clipped, onehot], dim=-1)
    return F.linear(x, weight_ih.to(feat.dtype), (bias_ih + bias_hh).to(feat.dtype))


class _CoreInputProjection(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, reward, prev_action, weight_ih, bias_ih, bias_hh):
        Xg = _kernels().lstm_input_fwd(feat, reward, prev_action, weight_ih, bias_ih, bias_hh)
        ctx.save_for_backward(feat, reward, prev_action, weight_ih)
        return Xg

    @staticmethod
    def backward(ctx, dXg):
        feat, reward, prev_action, weight_ih = ctx.saved_tensors
        d_feat, dW, db = _kernels().lstm_input_bwd(
            dXg.contiguous(), feat, reward, prev_action, weight_ih, ctx.needs_input_grad[0]
        )
        # dW and db are fp32; autograd casts them to the parameters' dtype
        return d_feat, None, None, dW, db, db


def core_input_projection(feat, reward, prev_action, weight_ih, bias_ih, bias_hh):
    """feat [M,256] (relu(fc(x))); reward [M], not clipped; prev_action [M], any
    integer dtype; weight_ih [4H, 257+A] in the model's column order (features,
    reward, actions); bias_ih, bias_hh [4H]. Returns Xg [M,4H]:

      Xg[m,n] = sum_k feat[m,k] W[n,k] + clamp(reward[m],-1,1) W[n,256]
                + W[n,257+a_m] + bias_ih[n] + bias_hh[n]

    On a GPU with _kernels built this is one launch (three more in the
    backward): feat bf16, W fp32 or bf16 and rounded to bf16 as it is read,
    fp32 accumulation with the reward in fp32, one rounding to the bf16 result.
    H in (128, 256, 512), A <= CORE_INPUT_MAX_ACTIONS; anything else on a GPU
    raises. Gradients: feat bf16, weight_ih and the biases fp32 (both biases
    get the same vector), none for reward and prev_action; summed in a fixed
    order. An action outside [0, A) contributes nothing. No host sync.
    On the CPU, or without _kernels, core_input_eager runs."""
    if not feat.is_cuda or _kernels() is None:
        return core_input_eager(feat, reward, prev_action, weight_ih, bias_ih, bias_hh)
    if feat.dim() != 2 or weight_ih.dim() != 2:
        raise ValueError("core_input_projection: feat [M,256] and weight_ih [4H,257+A] expected")
    A = weight_ih.shape[1] - feat.shape[1] - 1
    if not core_input_available(feat.shape[1], A, weight_ih.shape[0] // 4, feat.device):
        raise ValueError(
            "core_input_projection: no kernel for feature width %d, %d actions, weight_ih %s "
            "(width 256, 1..%d actions, hidden 128/256/512 are served)"
            % (feat.shape[1], A, tuple(weight_ih.shape), CORE_INPUT_MAX_ACTIONS)
        )
    if feat.dtype != torch.bfloat16:
        raise ValueError("core_input_projection: feat must be bf16 on the GPU, got %s" % feat.dtype)
    if not weight_ih.is_contiguous():
        raise ValueError("core_input_projection: weight_ih must be contiguous")
    return _CoreInputProjection.apply(
        feat.contiguous(), reward.contiguous(), prev_action.contiguous(), weight_ih, bias_ih, bias_hh
    )
