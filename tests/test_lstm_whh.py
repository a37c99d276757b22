"""The recurrent weight gradient and the W_hh pack (hip/lstm_whh.hip.inc), the
scan with native_whh=True, the AtariNet flag and the host checks.
docs/KERNEL_TESTS.md says why the weight-gradient tolerance is zero."""
import functools

import pytest
import torch

import kernel_refs as R
from test_lstm_wide import PRESENT

gpu = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

BF16 = torch.bfloat16
SIZES = [128, 256, 512]
# (T, B, notdone): notdone 0 or 1 fills the mask, None draws it at random
CASES = [
    (1, 1, 0),      # the only row is masked: all zeros although h0 is not
    (1, 1, 1),      # the only row is live: the outer product with h0
    (3, 33, None),  # B odd: row pairs straddle a step, the h0 -> H seam is inside
                    # a chunk, and the last chunk (99 = 64 + 35 rows) is ragged
]
# T*B = the slab length of the launch (5 * hidden rows) plus one row, B odd:
# two slabs, the second holding a single row
SLAB_PLUS_ONE = {
    128: (641, 1, None),   # slab 640
    256: (21, 61, None),   # slab 1280, 1281 = 21 * 61
    512: (13, 197, None),  # slab 2560, 2561 = 13 * 197
}
GRAD_CASES = [(h,) + c for h in SIZES for c in CASES + [SLAB_PLUS_ONE[h]]]


@functools.lru_cache(maxsize=None)
def grad_case(hidden, T, B, nd_value):
    """Integer inputs in [-4, 4] and the fp64 reference, computed once."""
    gen = torch.Generator().manual_seed(hidden + 7 * T + B)
    dG = R.int_tensor(gen, (T, B, 4 * hidden), -4, 4)
    H = R.int_tensor(gen, (T, B, hidden), -4, 4)
    h0 = R.int_tensor(gen, (B, hidden), -4, 4)
    if nd_value is None:
        nd = torch.randint(0, 2, (T, B), generator=gen).double()
        nd.view(-1)[0], nd.view(-1)[-1] = 0.0, 1.0
    else:
        nd = torch.full((T, B), float(nd_value), dtype=torch.float64)
        h0[0, 0] = 3.0
    Hp = torch.where(nd.unsqueeze(-1) != 0, torch.cat([h0.unsqueeze(0), H[:-1]]), 0.0)
    ref = dG.reshape(T * B, -1).t() @ Hp.reshape(T * B, -1)
    R.assert_int_exact(ref)
    return dG, H, h0, nd, ref


@gpu
@requires_gpu
@pytest.mark.parametrize("hidden,T,B,nd_value", GRAD_CASES)
def test_weight_grad_exact(hidden, T, B, nd_value):
    """Every product and partial sum is an integer far below 2**24, so fp32 in
    any order is exact: tolerance zero, and a second call agrees bit for bit."""
    from moolib_amd.ops.lstm import recurrent_weight_grad

    dG, H, h0, nd, ref = grad_case(hidden, T, B, nd_value)
    args = (dG.to(BF16).cuda(), H.to(BF16).cuda(), h0.to(BF16).cuda(), nd.float().cuda())
    dW = recurrent_weight_grad(*args)
    assert dW.dtype == torch.float32 and dW.shape == (4 * hidden, hidden)
    assert torch.equal(dW.cpu().double(), ref)
    if nd_value == 0:
        assert not ref.any()
    assert torch.equal(recurrent_weight_grad(*args), dW)


@gpu
@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float32, BF16])
@pytest.mark.parametrize("hidden", SIZES)
def test_pack_bit_equal(hidden, dtype):
    from moolib_amd.ops.lstm import pack_mfma_b, pack_whh

    torch.manual_seed(hidden)
    w = torch.randn(4 * hidden, hidden).to(dtype).cuda()
    packed_t, packed_n = pack_whh(w)
    assert packed_t.dtype == packed_n.dtype == BF16
    assert torch.equal(packed_t, pack_mfma_b(w.to(BF16).t().contiguous()))
    assert torch.equal(packed_n, pack_mfma_b(w.to(BF16).contiguous()))


@gpu
@requires_gpu
@pytest.mark.parametrize("hidden", SIZES)
def test_scan_native_whh(hidden):
    """Same scan kernels on the same packed bits: everything but dW is
    bit-identical to the default route; dW within test_lstm_wide's bound."""
    from moolib_amd.ops.lstm import fused_lstm_scan

    T, B = 3, 33
    d = R.lstm_inputs(torch.Generator().manual_seed(hidden + 100 * T + B), T, B, hidden=hidden)
    exact, emul = R.lstm_exact(d), R.lstm_emul(d)

    def run(native):
        X, h0 = (d[k].to(BF16).cuda().requires_grad_() for k in ("X", "h0"))
        c0, w = (d[k].float().cuda().requires_grad_() for k in ("c0", "w"))
        nd = d["nd"].float().cuda()
        H, hT, cT = fused_lstm_scan(X, nd, h0, c0, w, native_whh=native)
        ((H.float() * d["gH"].float().cuda()).sum() + (hT.float() * d["ghT"].float().cuda()).sum()
         + (cT * d["gcT"].float().cuda()).sum()).backward()
        with torch.no_grad():
            plain = fused_lstm_scan(X, nd, h0, c0, w, native_whh=native)
        return {"H": H.detach(), "hT": hT.detach(), "cT": cT.detach(), "dX": X.grad,
                "dh0": h0.grad, "dc0": c0.grad, "dW": w.grad}, plain

    native, native_plain = run(True)
    default, _ = run(False)
    for k in ("H", "hT", "cT", "dX", "dh0", "dc0"):
        assert torch.equal(native[k], default[k]), k
    for k, t in zip(("H", "hT", "cT"), native_plain):
        assert t.grad_fn is None and torch.equal(t, default[k]), k
    dist, bound = R.lstm_bounds(exact, emul)["dW"]
    atol, rel = PRESENT["dW"]
    bound = min(bound, atol + rel * exact["dW"].abs().max().item())
    err = (native["dW"].cpu().double() - exact["dW"]).abs().max().item()
    print("LSTM_WHH_FIGURE", hidden, "dW d=%.3g err=%.3g bound=%.3g" % (dist, err, bound))
    assert err <= bound


def test_weight_grad_cpu():
    from moolib_amd.ops.lstm import recurrent_weight_grad

    dG, H, h0, nd, ref = grad_case(128, 3, 5, None)
    dW = recurrent_weight_grad(dG.to(BF16), H.to(BF16), h0.to(BF16), nd.float())
    assert dW.dtype == torch.float32 and torch.equal(dW.double(), ref)


def test_flag_interface():
    from moolib_amd.models.atari import AtariNet, create_model

    shapes = lambda m: [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    default = AtariNet(num_actions=6, use_lstm=True)
    flagged = AtariNet(num_actions=6, use_lstm=True, fused_core_recurrent=True)
    assert shapes(flagged) == shapes(default)
    assert flagged.fused_core_recurrent and not default.fused_core_recurrent
    assert create_model(num_actions=6, use_lstm=True, fused_core_recurrent=True).fused_core_recurrent


@gpu
@requires_gpu
@pytest.mark.parametrize("why", ["hidden size 64", "dG not contiguous", "h0 dtype",
                                 "notdone shape", "pack hidden size 64", "pack dtype"])
def test_host_checks(why):
    from moolib_amd import _kernels

    T, B, Hd = 2, 3, 128
    z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device="cuda")
    dG, H, h0, nd = z(T, B, 4 * Hd), z(T, B, Hd), z(B, Hd), z(T, B, dt=torch.float32)
    _kernels.lstm_whh_grad(dG, H, h0, nd)  # the accepted forms
    _kernels.lstm_whh_pack(z(4 * Hd, Hd))
    bad = {
        "hidden size 64": (z(T, B, 256), z(T, B, 64), z(B, 64), nd),
        "dG not contiguous": (z(B, T, 4 * Hd).transpose(0, 1), H, h0, nd),
        "h0 dtype": (dG, H, z(B, Hd, dt=torch.float32), nd),
        "notdone shape": (dG, H, h0, z(B, T, dt=torch.float32)),
        "pack hidden size 64": (z(256, 64),),
        "pack dtype": (z(4 * Hd, Hd, dt=torch.float16),),
    }
    fn = _kernels.lstm_whh_pack if why.startswith("pack") else _kernels.lstm_whh_grad
    with pytest.raises(RuntimeError):
        fn(*bad[why])
