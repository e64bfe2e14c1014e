"""Sampled frame augmentation (csrc/augment.hip, safevla_amd/preproc.py) against an fp32 restatement of its arithmetic contract (DESIGN.md "Sampled frame
augmentation") written here in plain CPU torch.  torchvision is not a dependency: parity is pinned against this restatement, not against torchvision itself.

Criterion of every comparison: each stage is ONE rounding to u8 of a function that both sides compute in fp32 from identical u8 inputs, so the two can differ only
where the unrounded value sits on a rounding boundary and the two summation orders / divisions fall on either side of it: at most 1 level, on a small share of the
pixels.  The share is printed per stage and capped at 1 % on the noise input; an identity (factor 1.0 / hue 0 / whole-frame box / posterize) must be bit-exact.
The restatement's own fp32-versus-fp64 disagreement on these inputs (test_restatement_fp32_vs_fp64_cpu asserts it on the two small shapes: at most 1 level on at
most half the cap) was measured when this file was written: 0 for every stage except saturation 1.1873 (1.7e-4 of the noise values at 24 x 40) and crop + resize
(2.7e-3 at 9 x 37, where the interpolation weights are small fractions and exact .5 ties are common) -- far below the cap.  The jitter factors are deliberately not
short decimals: with brightness 0.7 every x that is a multiple of 10 puts 0.7 x on a truncation boundary, and the fp32 rounding of the product (not its real
value) decides a tenth of the pixels -- which is why the contract fixes fp32 and separately rounded operations, and the kernels are built without fp contraction.

The full chain is checked teacher-forced: the restatement of stage k is applied to the GPU's output of stage k - 1, so that a boundary case of one stage does not
decide the inputs of the next."""
import functools
import itertools
import random

import pytest
import torch
import torch.nn.functional as F

F32, F64, U8 = torch.float32, torch.float64, torch.uint8
SHAPES = [(3, 9, 37), (2, 24, 40), (2, 224, 384)]
CAP = 0.01


# ------------------------------------------------------------------------------------------------ the restatement (CPU, dtype dt = fp32; fp64 for the self-check)
def _t(v, dt):
    return torch.tensor(v, dtype=dt)


def r_blend(a, b, r, dt=F32):
    r = _t(r, dt) if not torch.is_tensor(r) else r
    return (r * a + (1 - r) * b).clamp(0, 255).trunc()


def r_gray(x, dt=F32):
    return (_t(0.2989, dt) * x[..., 0] + _t(0.587, dt) * x[..., 1] + _t(0.114, dt) * x[..., 2]).trunc()


def r_brightness(x_u8, f, dt=F32):
    x = x_u8.to(dt)
    return r_blend(x, torch.zeros_like(x), _t(f, F32).to(dt), dt).to(U8)


def r_contrast(x_u8, f, dt=F32):
    x = x_u8.to(dt)
    g = r_gray(x, dt)
    # the exact mean of the integer gray values of ONE image, rounded once to fp32
    m = (g.to(torch.int64).sum(dim=(1, 2)).to(F64) / (x.shape[1] * x.shape[2])).to(F32).to(dt)
    return r_blend(x, m[:, None, None, None], _t(f, F32).to(dt), dt).to(U8)


def r_saturation(x_u8, f, dt=F32):
    x = x_u8.to(dt)
    return r_blend(x, r_gray(x, dt)[..., None], _t(f, F32).to(dt), dt).to(U8)


def r_hue(x_u8, f, dt=F32):
    x = x_u8.to(dt) / 255
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    maxc, minc = x.max(-1).values, x.min(-1).values
    eq = maxc == minc
    cr = maxc - minc
    one = torch.ones_like(maxc)
    s = cr / torch.where(eq, one, maxc)
    dv = torch.where(eq, one, cr)
    rc, gc, bc = (maxc - r) / dv, (maxc - g) / dv, (maxc - b) / dv
    h = torch.where(maxc == r, bc - gc, torch.where(maxc == g, 2.0 + rc - bc, 4.0 + gc - rc))
    h = torch.fmod(h / 6.0 + 1.0, 1.0)
    h = torch.remainder(h + _t(f, F32).to(dt), 1.0)
    v = maxc
    h6 = h * 6.0
    fi = torch.floor(h6)
    fr = h6 - fi
    i = fi.to(torch.int64) % 6
    p = (v * (1.0 - s)).clamp(0, 1)
    q = (v * (1.0 - s * fr)).clamp(0, 1)
    t = (v * (1.0 - s * (1.0 - fr))).clamp(0, 1)
    tab = [(v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q)]
    out = torch.zeros_like(x)
    for k, trip in enumerate(tab):
        for c in range(3):
            out[..., c] = torch.where(i == k, trip[c], out[..., c])
    return (out * _t(255.999, F32).to(dt)).trunc().to(U8)


def r_gauss(ksize, sigma, dt=F32):
    half = (ksize - 1) * 0.5
    x = torch.linspace(-half, half, ksize, dtype=dt)
    pdf = torch.exp(-0.5 * (x / _t(sigma, F32).to(dt)).pow(2))
    return pdf / pdf.sum()


def r_blur(x_u8, sigma, dt=F32):
    x = x_u8.to(dt).permute(0, 3, 1, 2)
    k = r_gauss(9, sigma, dt)[:, None] * r_gauss(5, sigma, dt)[None, :]         # 9 high x 5 wide
    xp = F.pad(x, (2, 2, 4, 4), mode="reflect")
    y = F.conv2d(xp, k[None, None].expand(3, 1, 9, 5).contiguous(), groups=3)
    return y.round().clamp(0, 255).permute(0, 2, 3, 1).to(U8)


def _src(out, inn, dt):
    scale = _t(inn, F32) / _t(out, F32)                                           # fp32 on both sides
    s = ((torch.arange(out, dtype=F32) + 0.5) * scale - 0.5).clamp(min=0)
    i0 = s.floor().to(torch.int64).clamp(max=inn - 1)
    i1 = (i0 + 1).clamp(max=inn - 1)
    return i0, i1, (s - i0.to(F32)).to(dt)


def r_crop_resize(x_u8, box, dt=F32):
    top, left, bh, bw = box
    B, H, W, _ = x_u8.shape
    c = x_u8[:, top:top + bh, left:left + bw].to(dt)
    y0, y1, ly = _src(H, bh, dt)
    x0, x1, lx = _src(W, bw, dt)
    ly, lx = ly[None, :, None, None], lx[None, None, :, None]
    r0, r1 = c[:, y0], c[:, y1]
    v = (1 - ly) * ((1 - lx) * r0[:, :, x0] + lx * r0[:, :, x1]) + ly * ((1 - lx) * r1[:, :, x0] + lx * r1[:, :, x1])
    return v.round().clamp(0, 255).to(U8)


def r_posterize(x_u8, dt=F32):
    return x_u8 & 0xFE


def r_sharpness(x_u8, dt=F32):
    x = x_u8.to(dt).permute(0, 3, 1, 2)
    k = torch.ones(3, 3, dtype=dt)
    k[1, 1] = 5.0
    k = k / k.sum()
    bl = x.clone()
    bl[:, :, 1:-1, 1:-1] = F.conv2d(x, k[None, None].expand(3, 1, 3, 3).contiguous(), groups=3).round()
    return r_blend(x, bl, _t(2.0, dt), dt).permute(0, 2, 3, 1).to(U8)


R_JITTER = {0: r_brightness, 1: r_contrast, 2: r_saturation, 3: r_hue}


# ------------------------------------------------------------------------------------------------ inputs (computed once, never modified)
@functools.lru_cache(maxsize=None)
def frames(shape, kind):
    B, H, W = shape
    if kind == "noise":
        g = torch.Generator().manual_seed(1000 + H)
        return torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=U8)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    checker = (((yy + xx) % 2) * 255).to(U8)[..., None].expand(H, W, 3)
    return torch.stack([torch.zeros(H, W, 3, dtype=U8), torch.full((H, W, 3), 255, dtype=U8), checker]).contiguous()      # saturated: all 0 / all 255 / checkerboard


def box_for(shape):
    B, H, W = shape
    return (0, 42, 224, 299) if (H, W) == (224, 384) else (1, 3, H - 2, W - 5)


# stage name -> (restatement(x_u8, dt), gpu(x_u8 on the device), identity?)
def stage_table(shape):
    from safevla_amd import ops
    from safevla_amd.preproc import gaussian_weights
    B, H, W = shape
    tab = {}

    def jit(name, op, f, ident=False):
        def gpu(x):
            part = ops.aug_gray_partials(x) if op == 1 else None
            return ops.aug_jitter_blur(x, [op], [f], part)
        tab[name] = (lambda x, dt=F32: R_JITTER[op](x, f, dt), gpu, ident)

    jit("brightness_0.7123", 0, 0.7123); jit("brightness_1.3711", 0, 1.3711); jit("brightness_1.0", 0, 1.0, True)
    jit("contrast_0.6317", 1, 0.6317); jit("contrast_1.3931", 1, 1.3931)
    jit("saturation_0.8123", 2, 0.8123); jit("saturation_1.1873", 2, 1.1873); jit("saturation_1.0", 2, 1.0, True)
    jit("hue_-0.05", 3, -0.05); jit("hue_0.031", 3, 0.031); jit("hue_0", 3, 0.0, True)
    for sg in (0.1, 0.7, 2.0):
        tab[f"blur_{sg}"] = (lambda x, dt=F32, sg=sg: r_blur(x, sg, dt),
                             lambda x, sg=sg: ops.aug_jitter_blur(x, wx=gaussian_weights(5, sg), wy=gaussian_weights(9, sg)), False)
    bx = box_for(shape)
    tab["crop_resize"] = (lambda x, dt=F32: r_crop_resize(x, bx, dt), lambda x: ops.aug_resize_post_sharp(x, bx), False)
    tab["crop_whole_frame"] = (lambda x, dt=F32: r_crop_resize(x, (0, 0, H, W), dt), lambda x: ops.aug_resize_post_sharp(x, (0, 0, H, W)), True)
    tab["posterize"] = (lambda x, dt=F32: r_posterize(x), lambda x: ops.aug_resize_post_sharp(x, posterize=True), False)
    tab["sharpness"] = (lambda x, dt=F32: r_sharpness(x, dt), lambda x: ops.aug_resize_post_sharp(x, sharpen=True), False)
    return tab


STAGE_NAMES = ["brightness_0.7123", "brightness_1.3711", "brightness_1.0", "contrast_0.6317", "contrast_1.3931", "saturation_0.8123", "saturation_1.1873", "saturation_1.0",
               "hue_-0.05", "hue_0.031", "hue_0", "blur_0.1", "blur_0.7", "blur_2.0", "crop_resize", "crop_whole_frame", "posterize", "sharpness"]
EXACT = {"posterize", "brightness_1.0", "saturation_1.0", "hue_0", "crop_whole_frame"}


def compare(name, got_u8, ref_u8, cap=None, exact=False):
    d = (got_u8.cpu().to(torch.int16) - ref_u8.to(torch.int16)).abs()
    share = (d > 0).float().mean().item()
    print(f"{name}: max |diff| {int(d.max())}, differing share {share:.2e}")
    if exact:
        assert int(d.max()) == 0, f"{name}: must be bit-exact, {int((d > 0).sum())} values differ (max {int(d.max())})"
    assert int(d.max()) <= 1, f"{name}: max |diff| {int(d.max())} level(s)"
    if cap is not None:
        assert share <= cap, f"{name}: {share:.3%} of the values differ -- more than rounding-boundary cases"


@pytest.mark.parametrize("name", STAGE_NAMES)
def test_restatement_fp32_vs_fp64_cpu(name):
    """the yardstick's own noise floor: the restatement in fp32 against the same formulas in fp64, small and middle shape"""
    for shape in SHAPES[:2]:
        ref = stage_table(shape)[name][0]
        for kind in ("noise", "saturated"):
            x = frames(shape, kind)
            a, b = ref(x, F32), ref(x, F64)
            d = (a.to(torch.int16) - b.to(torch.int16)).abs()
            print(name, shape, kind, int(d.max()), f"{(d > 0).float().mean().item():.2e}")
            assert int(d.max()) <= 1 and (d > 0).float().mean().item() <= CAP / 2, (name, shape, kind, int(d.max()), (d > 0).float().mean().item())


# ------------------------------------------------------------------------------------------------ 1. each stage alone
@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", STAGE_NAMES)
def test_stage_alone(shape, name):
    ref, gpu, ident = stage_table(shape)[name]
    for kind in ("noise", "saturated"):
        x = frames(shape, kind)
        got = gpu(x.cuda())
        compare(f"{name} {kind} {shape}", got, ref(x), cap=CAP if kind == "noise" else None, exact=name in EXACT)
        if ident:
            assert torch.equal(got.cpu(), x), f"{name}: an identity must return its input bit for bit"
    if name == "posterize":
        assert torch.equal(gpu(frames(shape, "noise").cuda()).cpu(), frames(shape, "noise") & 0xFE)


# ------------------------------------------------------------------------------------------------ 2. / 3. full chain
def make_call(seed, order, shape, post=None, sharp=None):
    from safevla_amd.preproc import AugmentCall, sample_augment_params
    p = sample_augment_params(random.Random(seed))
    if post is not None:
        p = p._replace(posterize_draws=(0, int(post), 0, 0))
    if sharp is not None:
        p = p._replace(sharpness=int(sharp))
    return AugmentCall(p, tuple(order), box_for(shape))


def check_chain(x, call, tag):
    """debug form teacher-forced against the restatement, then the product form against the debug form's last stage, bit for bit"""
    from safevla_amd.preproc import apply_augment_u8
    xg = x.cuda()
    stages = apply_augment_u8(xg, call, debug=True)
    assert [n for n, _ in stages] == ["jitter0", "jitter1", "jitter2", "jitter3", "blur", "crop_resize", "posterize", "sharpness"]
    p, prev = call.params, x
    for k, (name, img) in enumerate(stages):
        if k < 4:
            op = call.order[k]
            ref = R_JITTER[op](prev, p.factor(op))
        elif name == "blur":
            ref = r_blur(prev, p.sigma)
        elif name == "crop_resize":
            ref = r_crop_resize(prev, call.box)
        elif name == "posterize":
            ref = r_posterize(prev) if p.posterize else prev
        else:
            ref = r_sharpness(prev) if p.sharpness else prev
        compare(f"{tag} {name}", img, ref, cap=CAP, exact=name == "posterize")
        prev = img.cpu()
    prod = apply_augment_u8(xg, call)
    assert torch.equal(prod, stages[-1][1]), f"{tag}: the fused launches differ from one launch per stage"
    return prod


@pytest.mark.gpu
def test_chain_teacher_forced_all_24_orders_small():
    shape = SHAPES[1]
    x = frames(shape, "noise")
    for n, order in enumerate(itertools.permutations(range(4))):
        check_chain(x, make_call(n, order, shape, post=n % 2, sharp=(n // 2) % 2), f"order {order}")


@pytest.mark.gpu
@pytest.mark.parametrize("seed,order,post,sharp", [(11, (2, 0, 3, 1), 1, 1), (12, (1, 3, 0, 2), 0, 0), (13, (3, 1, 2, 0), None, None)])
def test_chain_teacher_forced_full_size(seed, order, post, sharp):
    shape = SHAPES[2]
    check_chain(frames(shape, "noise"), make_call(seed, order, shape, post, sharp), f"seed {seed}")


@pytest.mark.gpu
def test_chain_odd_shape_and_saturated():
    for kind in ("noise", "saturated"):
        check_chain(frames(SHAPES[0], kind), make_call(3, (0, 1, 2, 3), SHAPES[0], 1, 1), f"9x37 {kind}")


# ------------------------------------------------------------------------------------------------ 4. / 5. repeatability, batch scope
@pytest.mark.gpu
def test_repeatable_and_batch_scope():
    from safevla_amd.preproc import apply_augment_u8
    shape = SHAPES[1]
    call = make_call(21, (0, 2, 1, 3), shape, 1, 1)
    dark = (frames(shape, "noise")[:1] // 4)
    x = torch.cat([frames(shape, "noise"), dark, frames(shape, "saturated")]).cuda()          # 6 images of very different gray means
    a, b = apply_augment_u8(x, call), apply_augment_u8(x, call)
    assert torch.equal(a, b), "two runs differ"
    perm = torch.tensor([4, 2, 0, 5, 1, 3], device=x.device)
    assert torch.equal(apply_augment_u8(x[perm].contiguous(), call), a[perm]), "permuting the batch does not permute the output"
    for i in range(x.shape[0]):                                                               # the contrast mean is per image: every image alone gives its batch result
        assert torch.equal(apply_augment_u8(x[i:i + 1].contiguous(), call)[0], a[i]), i


# ------------------------------------------------------------------------------------------------ 6. plumbing
def _aug(seed, **kw):
    from safevla_amd.preproc import DataAugmentationPreprocessor
    return DataAugmentationPreprocessor("rgb", "aug", use_augmentation=True, generator=torch.Generator().manual_seed(seed), **kw)


@pytest.mark.gpu
def test_process_is_normalize_of_augment():
    from safevla_amd import ops
    from safevla_amd.preproc import DINO_RGB_MEANS, DINO_RGB_STDS
    x = frames(SHAPES[2], "noise").cuda()
    random.seed(5)
    a = _aug(7).process({"rgb": x})
    random.seed(5)
    p = _aug(7)
    b = ops.normalize_u8(p.augment_u8(x), DINO_RGB_MEANS, DINO_RGB_STDS)
    assert a.dtype == torch.float32 and a.shape == x.shape and torch.equal(a, b)
    # the schedule: the same transform on the next call, another ColorJitter order
    random.seed(5)
    q = _aug(7)
    c1, _ = q.augment_u8_stages(x)
    c2, st = q.augment_u8_stages(x)
    assert c1.params == c2.params and len(st) == 8 and all(s.dtype == torch.uint8 and s.shape == x.shape for _, s in st)


@pytest.mark.gpu
def test_vit_preprocessor_with_augmenters():
    from safevla_amd import ops
    from safevla_amd.preproc import DinoViTPreprocessor
    B = 2
    x = torch.cat([frames(SHAPES[2], "noise"), frames(SHAPES[2], "noise").flip(1)]).cuda()      # camera-major: 2 cameras x 2 envs

    def vit(**kw):
        torch.manual_seed(0)
        return DinoViTPreprocessor("rgb", "rgb_dinov2", **kw)

    plain = vit()
    # no augmenter: the same launches as before -- the tokens of the trunk, pooled
    tok = torch.zeros(B, 2, 84, 384, device="cuda", dtype=torch.bfloat16)
    plain.process_tokens_all_cameras(x, tok)
    t = plain.vit.patch_tokens(x, plain.MEAN, plain.STD, crop_x=plain.CROP_X)
    want = torch.zeros_like(tok)
    for cam in range(2):
        ops.adaptive_pool_tokens(t[cam * B:(cam + 1) * B], B, 1, 16, 27, 384, 7, 12, cam=cam, ncam=2, tok_out=want)
    assert torch.equal(tok, want)
    # one augmenter: process and process_tokens equal the plain preprocessor fed the augmented frames
    random.seed(9)
    got = vit(augmenter=_aug(1)).process({"rgb": x[:B]})
    random.seed(9)
    assert torch.equal(got, plain.process({"rgb": _aug(1).augment_u8(x[:B])}))
    random.seed(9)
    g1 = torch.zeros_like(tok); vit(augmenter=_aug(1)).process_tokens(x[:B], g1, cam=1)
    random.seed(9)
    w1 = torch.zeros_like(tok); plain.process_tokens(_aug(1).augment_u8(x[:B]), w1, cam=1)
    assert torch.equal(g1, w1)
    # two augmenters, one per camera, each on its camera-major slice
    random.seed(9)
    g2 = torch.zeros_like(tok); vit(augmenter=[_aug(1), _aug(2)]).process_tokens_all_cameras(x, g2)
    random.seed(9)
    a0, a1 = _aug(1), _aug(2)
    xa = torch.cat([a0.augment_u8(x[:B]), a1.augment_u8(x[B:])])
    w2 = torch.zeros_like(tok); plain.process_tokens_all_cameras(xa, w2)
    assert torch.equal(g2, w2) and not torch.equal(g2, tok)


# ------------------------------------------------------------------------------------------------ 7. refusals
@pytest.mark.gpu
def test_refusals_launch_nothing():
    from safevla_amd import ops
    from safevla_amd._lib import SvlaError

    def refused(fn, x, **kw):
        out = torch.full_like(x, 77)
        with pytest.raises(SvlaError):
            fn(x, out=out, **kw)
        torch.cuda.synchronize()
        assert bool((out == 77).all()), "a refused call wrote to its output"

    w5, w9 = [0.2] * 5, [1 / 9] * 9
    for shape in ((1, 4, 16, 3), (1, 16, 2, 3)):                                     # H < 5, W < 3
        x = torch.zeros(shape, dtype=U8, device="cuda")
        refused(ops.aug_jitter_blur, x, ops=[0], factors=[1.2], wx=w5, wy=w9)
        refused(ops.aug_resize_post_sharp, x, sharpen=True)
        with pytest.raises(SvlaError):
            ops.aug_gray_partials(x)
    x = torch.zeros(1, 16, 16, 3, dtype=U8, device="cuda")
    for box in ((0, 0, 17, 16), (0, 1, 16, 16), (-1, 0, 8, 8), (4, 4, 0, 8), (10, 10, 8, 8)):      # crop box outside the image
        refused(ops.aug_resize_post_sharp, x, box=box)
    y = ops.aug_resize_post_sharp(x + 3, box=(8, 8, 8, 8))                            # the largest legal corner box is served
    assert bool((y == 3).all())
