"""The split-K conv weight-gradient kernel (hip/wgrad3x3_splitk.hip.inc) and
its route MOOLIB_AMD_WGRAD_KERNEL=2, against float64 (docs/KERNEL_TESTS.md)."""
import pytest
import torch
from torch import nn

import kernel_refs as R

gpu = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X")

BF16 = torch.bfloat16
CASES = [(8, 4, 16), (8, 8, 16), (16, 16, 16), (16, 16, 32), (32, 32, 32), (32, 32, 16)]
# all halo; under one chunk, odd; the last section; W < 32 with a tail; one past a
# chunk; two chunks; three chunks and many slabs; None: (5, 2R+1, 16) for the host's R
SHAPES = [(1, 1, 1), (2, 3, 5), (1, 11, 11), (3, 21, 21), (2, 9, 33), (1, 42, 42), (1, 84, 84),
          None]


def kernels():
    from moolib_amd import _kernels

    return _kernels


def nhwc(t):
    return t.to(BF16).cuda().contiguous(memory_format=torch.channels_last)


@gpu
@requires_gpu
@pytest.mark.parametrize("want_db", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("C,c_real,K", CASES)
def test_exact(C, c_real, K, shape, want_db):
    k = kernels()
    if shape is None:
        rows = k.wgrad3x3_splitk_rows(C, K, 16)
        assert 1 <= rows <= 8
        shape = (5, 2 * rows + 1, 16)
    N, H, W = shape
    gen = torch.Generator().manual_seed(1000 * C + 10 * K + H + W)
    x = R.int_tensor(gen, (N, C, H, W), -2, 2)  # the padded channels too: they must not leak
    dy = R.int_tensor(gen, (N, K, H, W), -2, 2)
    ref = R.conv3x3_wgrad_ref(x[:, :c_real], dy)
    R.assert_int_exact(ref)
    dw, db = k.wgrad3x3_splitk(nhwc(x), nhwc(dy), c_real, want_db)
    assert dw.shape == (K, c_real, 3, 3) and dw.dtype == torch.float32
    assert torch.equal(dw.cpu().double(), ref)
    if want_db:
        assert db.dtype == torch.float32
        assert torch.equal(db.cpu().double(), dy.sum((0, 2, 3)))
    else:
        assert db.numel() == 0


@gpu
@requires_gpu
@pytest.mark.parametrize("N,H,W,C,K", [(3, 21, 21, 32, 32), (1, 84, 84, 8, 16)])
def test_bit_reproducible(N, H, W, C, K):
    k = kernels()
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(N, C, H, W, generator=gen).to(BF16)
    dy = torch.randn(N, K, H, W, generator=gen).to(BF16)
    a = k.wgrad3x3_splitk(nhwc(x), nhwc(dy), C, True)
    b = k.wgrad3x3_splitk(nhwc(x), nhwc(dy), C, True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # an fp32 sum of n exact bf16 products, in any order: n u sum|terms|, u = 2^-24
    n, u = N * H * W, 2.0 ** -24
    for got, ref, mag in (
        (a[0], R.conv3x3_wgrad_ref(x, dy), R.conv3x3_wgrad_ref(x.abs(), dy.abs())),
        (a[1], dy.double().sum((0, 2, 3)), dy.double().abs().sum((0, 2, 3))),
    ):
        err = (got.cpu().double() - ref).abs()
        print("max err %.3e, max bound %.3e" % (err.max(), (mag * n * u).max()))
        assert (err <= mag * n * u).all()


@gpu
@requires_gpu
def test_route(monkeypatch):
    from moolib_amd.ops import conv3x3 as C3

    assert hasattr(kernels(), "wgrad3x3_splitk")
    gen = torch.Generator().manual_seed(11)
    g32 = R.int_tensor(gen, (2, 32, 9, 33), -2, 2)
    x16 = R.int_tensor(gen, (2, 16, 9, 33), -2, 2)
    conv = nn.Conv2d(16, 32, 3, padding=1).cuda()
    conv.weight.data.copy_(R.int_tensor(gen, (32, 16, 3, 3), -1, 1))
    g16 = R.int_tensor(gen, (2, 16, 12, 20), -2, 2)
    frames = torch.randint(0, 4, (2, 4, 12, 20), generator=gen).to(torch.uint8)
    conv1 = nn.Conv2d(4, 16, 3, padding=1).cuda()
    conv1.weight.data.copy_(R.int_tensor(gen, (16, 4, 3, 3), -1, 1))
    conv1.bias.data.copy_(R.int_tensor(gen, (16,), -1, 1))

    grads = {}
    for env in ("2", "1"):
        monkeypatch.setenv("MOOLIB_AMD_WGRAD_KERNEL", env)
        for m in (conv, conv1):
            m.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=BF16):
            y = C3.conv3x3_autograd(nhwc(x16), conv)
            y1 = C3.conv1_u8_autograd(frames.cuda(), conv1, 1.0)
        y.backward(g32.cuda().to(y.dtype))
        y1.backward(g16.cuda().to(y1.dtype))
        grads[env] = [conv.weight.grad.cpu(), conv1.weight.grad.cpu(), conv1.bias.grad.cpu()]
    refs = [R.conv3x3_wgrad_ref(x16, g32), R.conv3x3_wgrad_ref(frames.double(), g16),
            g16.sum((0, 2, 3))]
    R.assert_int_exact(*refs)
    for got, old, ref in zip(grads["2"], grads["1"], refs):
        assert got.dtype == torch.float32 and torch.equal(got, ref.float())
        assert torch.equal(old, got)
