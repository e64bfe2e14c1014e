"""Kernels of the frozen CLIP RN50 trunk (csrc/conv.hip) against torch.nn.functional on the CPU in fp32: the implicit-GEMM convolution (3x3 and 1x1, three
epilogues), its border handling, the fused u8 stem, AvgPool2d(2) and the argument checks.

Convolution bound: both sides use the same bf16-rounded operands upcast to fp32, so only the summation order and the final bf16 rounding differ:
|got - want| <= 2^-7 |want| + 1e-3 max|want| elementwise (bf16 half-ulp is 2^-9)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
EPIS = ("bias", "relu", "res_relu")


def _ops():
    from safevla_amd import ops
    return ops


def bf16r(x):
    return x.to(BF16).float()


def conv_case(B, H, W, Cin, Cout, taps, epi, seed=0):
    g = torch.Generator().manual_seed(seed)
    k = 3 if taps == 9 else 1
    x = bf16r(torch.randn(B, H, W, Cin, generator=g))
    w = bf16r(torch.randn(Cout, Cin, k, k, generator=g) / (Cin * taps) ** 0.5)
    b = torch.randn(Cout, generator=g)
    res = bf16r(torch.randn(B, H, W, Cout, generator=g)) if epi == "res_relu" else None
    return x, w, b, res


def conv_oracle(x, w, b, res, epi):
    y = F.conv2d(x.permute(0, 3, 1, 2), w, b, padding=w.shape[-1] // 2).permute(0, 2, 3, 1)
    if epi == "res_relu":
        y = y + res
    return F.relu(y) if epi != "bias" else y


def conv_gpu(x, w, b, res, epi, **kw):
    ops = _ops()
    B, H, W, Cin = x.shape
    Cout, taps = w.shape[0], w.shape[2] * w.shape[3]
    wk = w.permute(0, 2, 3, 1).reshape(Cout, taps, Cin).to(BF16).contiguous().to(DEV)
    y = ops.conv_nhwc(x.to(BF16).to(DEV), wk, b.to(DEV), B, H, W, taps, EPIS.index(epi), residual=None if res is None else res.to(BF16).to(DEV).reshape(-1, Cout), **kw)
    torch.cuda.synchronize()
    return y.float().cpu().reshape(B, H, W, Cout)


def assert_conv_close(got, want):
    tol = 2.0 ** -7 * want.abs() + 1e-3 * want.abs().max()
    err = (got - want).abs()
    print(f"max |err| {float(err.max()):.3e}, max |want| {float(want.abs().max()):.3e}, worst err / tol {float((err / tol).max()):.3f}")
    assert torch.isfinite(got).all() and bool((err <= tol).all()), float((err / tol).max())


SHAPES_3x3 = [(1, 5, 9, 32, 32), (2, 7, 12, 64, 64), (3, 8, 8, 128, 128), (1, 16, 16, 512, 512)]


@pytest.mark.parametrize("epi", EPIS)
@pytest.mark.parametrize("shape", SHAPES_3x3, ids=lambda s: "x".join(map(str, s)))
def test_conv3x3_vs_conv2d(shape, epi):
    """odd sizes below one tile; the 7 x 12 grid with a tile across rows and the image boundary; three images; K = 4608, the deepest reduction of the network"""
    x, w, b, res = conv_case(*shape, 9, epi, seed=sum(shape))
    assert_conv_close(conv_gpu(x, w, b, res, epi), conv_oracle(x, w, b, res, epi))


@pytest.mark.parametrize("shape,epi", [((2, 7, 12, 256, 64), "bias"), ((2, 7, 12, 256, 64), "relu"), ((2, 7, 12, 64, 256), "res_relu")],
                         ids=["256to64-bias", "256to64-relu", "64to256-res_relu"])
def test_conv1x1_vs_conv2d(shape, epi):
    """the 1x1 form: N = 64 (the two layer1 convolutions the GEMM does not take) and the block's last convolution with ReLU(out + identity)"""
    x, w, b, res = conv_case(*shape, 1, epi, seed=7)
    assert_conv_close(conv_gpu(x, w, b, res, epi), conv_oracle(x, w, b, res, epi))


def test_conv_output_row_map_writes_one_camera_slot():
    """y_group / y_group_stride: the rows of image b go to out[b, cam] of a [B, ncam, H*W, Cout] tensor, the other slot keeps its sentinel"""
    B, H, W, Cin, Cout = 3, 2, 3, 32, 64
    x, w, b, res = conv_case(B, H, W, Cin, Cout, 1, "res_relu", seed=3)
    out = torch.full((B, 2, H * W, Cout), -7.0, device=DEV, dtype=BF16)
    conv_gpu(x, w, b, res, "res_relu", out=out[:, 1], ldy=Cout, y_group=H * W, y_group_stride=2 * H * W)
    want = conv_oracle(x, w, b, res, "res_relu")
    assert bool((out[:, 0] == -7.0).all())
    assert_conv_close(out[:, 1].float().cpu().reshape(B, H, W, Cout), want)


@pytest.mark.parametrize("hw", [(6, 9), (1, 5), (4, 1)], ids=lambda s: "x".join(map(str, s)))
def test_conv3x3_does_not_leak_across_rows_or_images(hw):
    """Image 0 all zeros, image 1 all ones, integer weights and bias: every sum is an exact small integer whatever the summation order, so the output must EQUAL the
    oracle -- at every border pixel of both images (asserted on its own) and everywhere else.  One tile holds both images: a kernel that reads the next row's or the
    next image's pixel for an out-of-image neighbour gets a different integer."""
    H, W = hw
    Cin = Cout = 32
    g = torch.Generator().manual_seed(H * 31 + W)
    x = torch.cat([torch.zeros(1, H, W, Cin), torch.ones(1, H, W, Cin)])
    w = torch.randint(-1, 2, (Cout, Cin, 3, 3), generator=g).float()
    b = torch.randint(-2, 3, (Cout,), generator=g).float()
    want = conv_oracle(x, w, b, None, "bias")
    assert torch.equal(want, bf16r(want)) and float(want[1].abs().max()) > 8      # the oracle itself is bf16-exact, and not trivial
    got = conv_gpu(x, w, b, None, "bias")
    border = torch.zeros(H, W, dtype=torch.bool)
    border[0], border[-1], border[:, 0], border[:, -1] = True, True, True, True
    assert torch.equal(got[:, border], want[:, border]), (got[:, border] - want[:, border]).abs().max()
    assert torch.equal(got[0], b.expand(H, W, Cout))                                # nothing of image 1 reaches image 0
    assert torch.equal(got, want)


@pytest.mark.parametrize("shape", [(2, 30, 44), (1, 31, 45)], ids=lambda s: "x".join(map(str, s)))
def test_stem_vs_normalise_conv_bn_relu(shape):
    """u8 frame -> (x / 255 - mean) / std -> conv2d(stride 2, padding 1) -> BatchNorm (eval) -> ReLU; the kernel takes the folded weights.  31 x 45: odd sizes,
    output 16 x 23"""
    from safevla_amd.preproc import CLIP_RGB_MEANS, CLIP_RGB_STDS
    B, H, W = shape
    g = torch.Generator().manual_seed(H)
    fr = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    w = torch.randn(32, 3, 3, 3, generator=g) / 27 ** 0.5
    gamma, beta = 1 + 0.2 * torch.randn(32, generator=g), 0.1 * torch.randn(32, generator=g)
    mean, var = 0.1 * torch.randn(32, generator=g), 0.5 + torch.rand(32, generator=g)
    xn = (fr.permute(0, 3, 1, 2).float() / 255.0 - torch.tensor(CLIP_RGB_MEANS).view(1, 3, 1, 1)) / torch.tensor(CLIP_RGB_STDS).view(1, 3, 1, 1)
    want = F.relu(F.batch_norm(F.conv2d(xn, w, stride=2, padding=1), mean, var, gamma, beta, False, 0.0, 1e-5)).permute(0, 2, 3, 1)
    s = gamma / torch.sqrt(var + 1e-5)
    wk = (w * s[:, None, None, None]).permute(2, 3, 1, 0).reshape(27, 32).contiguous()
    got = _ops().conv_stem_u8(fr.to(DEV), CLIP_RGB_MEANS, CLIP_RGB_STDS, wk.to(DEV), (beta - mean * s).to(DEV))
    torch.cuda.synchronize()
    assert tuple(got.shape) == (B, (H + 1) // 2, (W + 1) // 2, 32) == tuple(want.shape)
    assert_conv_close(got.float().cpu(), want)


@pytest.mark.parametrize("shape", [(2, 6, 10, 64), (1, 7, 13, 32)], ids=lambda s: "x".join(map(str, s)))
def test_avgpool2_vs_avg_pool2d(shape):
    """AvgPool2d(2) with floor semantics (7 x 13 -> 3 x 6); the bound is the output's bf16 rounding, 2^-8 relative"""
    B, H, W, C = shape
    x = bf16r(torch.randn(B, H, W, C, generator=torch.Generator().manual_seed(C)))
    want = F.avg_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    got = _ops().avgpool2_nhwc(x.to(BF16).to(DEV), B, H, W, C)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (B, H // 2, W // 2, C) == tuple(want.shape)
    assert bool(((got.float().cpu() - want).abs() <= 2.0 ** -8 * want.abs()).all())


@pytest.mark.parametrize("cin,cout,taps", [(48, 64, 9), (64, 48, 9), (64, 64, 4), (64, 64, 3)], ids=["cin48", "cout48", "taps4", "taps3"])
def test_conv_refuses_unsupported_arguments(cin, cout, taps):
    """a channel count that is not a multiple of 32, or a tap count other than 1 / 9: SVLA_EINVAL, nothing launched, the output keeps its sentinel"""
    from safevla_amd._lib import lib
    B, H, W = 1, 4, 4
    x = torch.zeros(B * H * W, cin, device=DEV, dtype=BF16)
    w = torch.zeros(cout, taps, cin, device=DEV, dtype=BF16)
    b = torch.zeros(cout, device=DEV)
    y = torch.full((B * H * W, cout), 3.0, device=DEV, dtype=BF16)
    rc = lib().cdll.svla_conv_nhwc_bf16(x.data_ptr(), w.data_ptr(), b.data_ptr(), None, 0, y.data_ptr(), cout, 0, 0, B, H, W, cin, cout, taps, 0, None)
    torch.cuda.synchronize()
    assert rc == -1 and bool((y == 3.0).all())
    with pytest.raises(RuntimeError):
        _ops().conv_nhwc(x, w, b, B, H, W, taps, out=y)
