"""Antialiased bicubic u8 resize (csrc/resize.hip, ops.resize_bicubic_aa_u8) and the camera-frame front of the SigLIP presets
(preproc.SigLIPDataAugmentationPreprocessor) against torch's own CPU ``F.interpolate(..., mode="bicubic", antialias=True)`` evaluated in fp64.

Criterion of the kernel comparison: the kernel computes in fp32 what the oracle computes in fp64 and both round once, so they may differ only where the unrounded
value sits on a rounding boundary.  fp32 accumulation over at most 8 x 8 taps of values up to 255 carries an error of a few 1e-4: a pixel must be EQUAL wherever the
fp64 value is farther than 2e-3 from a half-integer and may differ by one level elsewhere (about 2e-3 of the noise pixels lie inside that window; torch's own fp32
result meets the same condition against its fp64 result, so the window cannot hide a wrong tap)."""
import random

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
U8 = torch.uint8
WINDOW = 2e-3
GEOMS = [(14, 24, 16, 16),        # the camera's own ratios 0.875 and 1.5 at one sixteenth size
         (28, 48, 32, 32),
         (37, 53, 16, 16),        # both axes shrink, odd tap counts
         (9, 11, 31, 29),         # both axes grow
         (224, 384, 256, 256)]
KINDS = ("noise", "smooth", "const255", "const0", "vstep", "hstep")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _inputs(B, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    ph = torch.arange(B * 3, dtype=torch.float64).reshape(B, 1, 1, 3)
    smooth = (127.5 + 127.5 * torch.sin(yy[None, :, :, None] * 0.21 + ph) * torch.cos(xx[None, :, :, None] * 0.13 - 0.5 * ph)).round().to(U8)
    vstep = torch.zeros(B, H, W, 3, dtype=U8)
    vstep[:, :, W // 2:] = 255        # a vertical edge: 0 | 255 along x
    hstep = torch.zeros(B, H, W, 3, dtype=U8)
    hstep[:, H // 2:] = 255
    return {"noise": torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=U8), "smooth": smooth, "const255": torch.full((B, H, W, 3), 255, dtype=U8),
            "const0": torch.zeros(B, H, W, 3, dtype=U8), "vstep": vstep, "hstep": hstep}


def _oracle(x_u8, oh, ow):
    """(unrounded clamped fp64 [B,OH,OW,3], its rounding to u8): CPU F.interpolate in fp64"""
    v = F.interpolate(x_u8.permute(0, 3, 1, 2).double(), size=(oh, ow), mode="bicubic", antialias=True, align_corners=False).clamp(0, 255).permute(0, 2, 3, 1).contiguous()
    return v, v.round().to(U8)


def _meets(got, x_u8, oh, ow):
    """the criterion of the module docstring: equal outside the window, at most one level inside it"""
    v, want = _oracle(x_u8, oh, ow)
    d = (got.cpu().int() - want.int()).abs()
    far = ((v - v.floor()) - 0.5).abs() > WINDOW
    return tuple(got.shape) == tuple(want.shape) and int(d.max()) <= 1 and int((d[far] > 0).sum()) == 0


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "%dx%d-%dx%d" % g)
def test_kernel_vs_fp64_interpolate(geom, B):
    _need_gpu()
    from safevla_amd import ops
    H, W, OH, OW = geom
    for kind, x in _inputs(B, H, W, seed=H * 1000 + W + B).items():
        v, want = _oracle(x, OH, OW)
        got = ops.resize_bicubic_aa_u8(x.to(DEV), (OH, OW)).cpu()
        assert got.shape == want.shape and got.dtype == U8
        d = (got.int() - want.int()).abs()
        far = ((v - v.floor()) - 0.5).abs() > WINDOW
        print(f"[{H}x{W}->{OH}x{OW} B={B} {kind}] differing {int((d > 0).sum())} of {d.numel()}, max {int(d.max())}, inside the window {float((~far).double().mean()):.2e}")
        assert int(d.max()) <= 1, (kind, int(d.max()))
        assert int((d[far] > 0).sum()) == 0, (kind, int((d[far] > 0).sum()))
        if kind.startswith("const"):
            assert bool((got == x[0, 0, 0, 0]).all()), kind
        if kind in ("vstep", "hstep"):      # the edge overshoots on both sides and is clamped
            assert int(got.min()) == 0 and int(got.max()) == 255


def test_identity_out_and_argument_checks():
    _need_gpu()
    from safevla_amd import ops
    g = torch.Generator().manual_seed(3)
    for H, W in [(16, 16), (37, 53), (224, 384)]:
        x = torch.randint(0, 256, (2, H, W, 3), generator=g, dtype=U8).to(DEV)
        assert torch.equal(ops.resize_bicubic_aa_u8(x, (H, W)), x)
    x = torch.randint(0, 256, (2, 14, 24, 3), generator=g, dtype=U8).to(DEV)
    out = torch.full((2, 16, 16, 3), 7, dtype=U8, device=DEV)
    r = ops.resize_bicubic_aa_u8(x, (16, 16), out=out)
    assert r is out and _meets(out, x.cpu(), 16, 16)
    # one axis only: the other keeps its single-tap weights
    one = ops.resize_bicubic_aa_u8(x, (14, 16))
    assert _meets(one, x.cpu(), 14, 16)
    assert torch.equal(one, ops.resize_bicubic_aa_u8(x.transpose(1, 2).contiguous(), (16, 14)).transpose(1, 2))      # the same taps on the other axis
    out.fill_(7)
    with pytest.raises(ValueError):
        ops.resize_bicubic_aa_u8(x.transpose(1, 2), (16, 16), out=out)                # not contiguous
    with pytest.raises(TypeError):
        ops.resize_bicubic_aa_u8(x.float(), (16, 16), out=out)
    with pytest.raises(ValueError):
        ops.resize_bicubic_aa_u8(x.cpu(), (16, 16), out=out)                          # host tensor
    with pytest.raises(ValueError):
        ops.resize_bicubic_aa_u8(x, (16, 16), out=torch.empty(2, 16, 17, 3, dtype=U8, device=DEV))
    torch.cuda.synchronize()
    assert bool((out == 7).all())


def test_refusals_launch_nothing():
    _need_gpu()
    from safevla_amd import ops
    from safevla_amd._lib import SvlaError
    x = torch.zeros(1, 16, 40, 3, dtype=U8, device=DEV)

    def refused(fn, out):
        with pytest.raises(SvlaError):
            fn(out)
        torch.cuda.synchronize()
        assert bool((out == 7).all())

    seven = lambda *s: torch.full(s, 7, dtype=U8, device=DEV)
    refused(lambda o: ops.resize_bicubic_aa_u8(x, (16, 8), out=o), seven(1, 16, 8, 3))          # 40 -> 8: scale 5
    refused(lambda o: ops.resize_bicubic_aa_u8(x, (68, 40), out=o), seven(1, 68, 40, 3))        # 16 -> 68: scale below 1/4
    refused(lambda o: ops.resize_bicubic_aa_u8(x[:, :8], (3, 40), out=o), seven(1, 3, 40, 3))   # OH < 4
    refused(lambda o: ops.lib().call("svla_resize_bicubic_aa_u8", x.data_ptr(), o.data_ptr(), 0, 16, 40, 16, 16, 0), seven(1, 16, 16, 3))      # B = 0
    # the limits themselves are accepted
    assert ops.resize_bicubic_aa_u8(x, (4, 10)).shape == (1, 4, 10, 3) and ops.resize_bicubic_aa_u8(x, (64, 160)).shape == (1, 64, 160, 3)
    lim = torch.randint(0, 256, (2, 16, 40, 3), generator=torch.Generator().manual_seed(5), dtype=U8)
    for hw in [(4, 10), (64, 160), (4, 160)]:
        assert _meets(ops.resize_bicubic_aa_u8(lim.to(DEV), hw), lim, *hw), hw


def test_preprocessor_resize_normalise_and_augment():
    _need_gpu()
    from safevla_amd import ops
    from safevla_amd.preproc import AugmentCall, SigLIPDataAugmentationPreprocessor, apply_augment_u8, crop_box, sample_augment_params
    g = torch.Generator().manual_seed(11)
    x = torch.randint(0, 256, (3, 14, 24, 3), generator=g, dtype=U8).to(DEV)
    p = SigLIPDataAugmentationPreprocessor("rgb", "rgb_aug", device=DEV, height=14, width=24, size=(16, 16))
    want = ops.resize_bicubic_aa_u8(x, (16, 16))
    assert torch.equal(p.augment_u8(x), want)
    same = torch.randint(0, 256, (2, 16, 16, 3), generator=g, dtype=U8).to(DEV)
    assert p.augment_u8(same) is same                                                         # already the model's size: untouched
    out = p.process({"rgb": x})
    assert out.dtype == torch.float32 and tuple(out.shape) == (3, 16, 16, 3)
    assert float((out - (want.float() / 255 - 0.5) / 0.5).abs().max()) <= 1e-6
    assert tuple(p.observation_space.shape) == (16, 16, 3)
    # sampled augmentation at the resized geometry: the same draws, replayed by hand
    random.seed(21)
    pa = SigLIPDataAugmentationPreprocessor("rgb", "rgb_aug", device=DEV, height=14, width=24, size=(16, 16), use_augmentation=True,
                                            generator=torch.Generator().manual_seed(4))
    got = pa.augment_u8(x)
    random.seed(21)
    params = sample_augment_params()
    g2 = torch.Generator().manual_seed(4)
    order = tuple(int(v) for v in torch.randperm(4, generator=g2).tolist())
    call = AugmentCall(params, order, crop_box(16, 16, params.scale, g2))
    assert tuple(got.shape) == (3, 16, 16, 3) and torch.equal(got, apply_augment_u8(want, call))


def test_siglip_preprocessor_takes_camera_frames_through_the_augmenter_slot():
    _need_gpu()
    from safevla_amd import ops
    from safevla_amd.preproc import SigLIPDataAugmentationPreprocessor, SigLIPPreprocessor
    g = torch.Generator().manual_seed(13)
    B = 2
    frames = torch.randint(0, 256, (2 * B, 224, 384, 3), generator=g, dtype=U8).to(DEV)       # camera-major: B of camera 0, then B of camera 1
    resized = ops.resize_bicubic_aa_u8(frames, (256, 256))
    torch.manual_seed(0)
    plain = SigLIPPreprocessor("rgb", "rgb_siglip", device=DEV)
    with pytest.raises(AssertionError):
        plain.process({"rgb": frames[:1]})                                                    # without an augmenter 224 x 384 is still refused
    front = SigLIPPreprocessor("rgb", "rgb_siglip", device=DEV,
                               augmenter=[SigLIPDataAugmentationPreprocessor("rgb", "a0", device=DEV), SigLIPDataAugmentationPreprocessor("manip", "a1", device=DEV)])
    front.vit.load_state_dict(plain.vit.state_dict())
    tok = lambda: torch.zeros(B, 2, 84, 768, device=DEV, dtype=torch.bfloat16)
    want, got, got_all = tok(), tok(), tok()
    for cam in range(2):
        plain.process_tokens(resized[cam * B:(cam + 1) * B], want, cam)
        front.process_tokens(frames[cam * B:(cam + 1) * B], got, cam)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    want_all = tok()
    plain.process_tokens_all_cameras(resized, want_all)
    front.process_tokens_all_cameras(frames, got_all)
    assert torch.equal(got_all.view(torch.int16), want_all.view(torch.int16))
    assert float(want_all.float().abs().max()) > 0
