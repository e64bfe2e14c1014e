"""Per-trajectory random frame augmentation (the grouped kernels of csrc/augment.hip, preproc.apply_random_augment_u8): one transform per group of frames, three launches
whatever the number of groups.

The oracle is the single-transform path (preproc.apply_augment_u8), itself verified against its fp32 restatement in tests/test_augment_gpu.py: a grouped application
must equal, BIT FOR BIT, G applications of apply_augment_u8 on the G slices with the same order, factors, sigma, box and flags -- the kernels share their
arithmetic and are built without fp contraction, so there is no tolerance.  The old path knows posterize to 7 bits only (mask 0xFE); the masks 0xFC / 0xF8 / 0xF0 are
checked on a transform that is otherwise the identity, where the expected output is the input & mask."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
U8 = torch.uint8
# (groups, frames per group, H, W): W * 3 not a multiple of 4 and one row tile; a middle size; square (the crop search succeeds: a different box per group); the
# camera's size (three column tiles, 14 row tiles, the fallback box)
SHAPES = [(3, 2, 9, 37), (2, 3, 24, 40), (4, 1, 64, 64), (2, 1, 224, 384)]
ORDERS = [(1, 0, 2, 3), (0, 2, 3, 1), (3, 1, 0, 2), (2, 0, 1, 3)]      # contrast first, contrast last, two with contrast inside
POST = [0xFF, 0xFE, 0xFF, 0xFE]                                        # group 0: every optional stage off; posterize on in one group and off in the next
SHARP = [False, True, True, False]


def _calls(shape):
    """per-group transforms: factors and sigma as the sampler draws them (seeded), order / posterize / sharpness set per group as the lists above say; the box is
    the sampler's where the search can succeed or must fall back (64 x 64, 224 x 384) and a different hand-made one per group at the two small sizes"""
    from safevla_amd.preproc import sample_random_augment_call
    G, L, H, W = shape
    g = torch.Generator().manual_seed(100 + H)
    calls = []
    for k in range(G):
        c = sample_random_augment_call(H, W, g)._replace(order=ORDERS[k % 4], post_mask=POST[k % 4], sharpen=SHARP[k % 4])
        if H < 64:
            c = c._replace(box=[(0, 0, H, W), (1, 3, H - 2, W - 5), (2, 0, H - 3, W - 1)][k % 3])
        calls.append(c)
    return calls


@functools.lru_cache(maxsize=None)
def case(shape):
    """(frames on the device, calls, grouped result, per-slice result of the single-transform path) -- computed once, never modified"""
    from safevla_amd.preproc import apply_augment_u8, apply_random_augment_u8
    G, L, H, W = shape
    x = torch.randint(0, 256, (G * L, H, W, 3), generator=torch.Generator().manual_seed(2000 + H), dtype=U8).cuda()
    x[0] //= 4                                                          # a dark frame: the contrast mean is per image, also inside a group
    calls = _calls(shape)
    got = apply_random_augment_u8(x, calls, L)
    want = torch.cat([apply_augment_u8(x[k * L:(k + 1) * L].contiguous(), c.as_augment_call()) for k, c in enumerate(calls)])
    return x, calls, got, want


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_grouped_equals_single_transform_path_per_slice(shape):
    x, calls, got, want = case(shape)
    G, L, H, W = shape
    assert got.shape == x.shape and got.dtype == U8
    for k in range(G):
        d = (got[k * L:(k + 1) * L] != want[k * L:(k + 1) * L])
        assert not bool(d.any()), f"group {k} ({calls[k]}): {int(d.sum())} values differ from apply_augment_u8 on its slice"
    assert not torch.equal(got, x)
    boxes = {c.box for c in calls}
    if (H, W) == (64, 64):
        assert len(boxes) >= 2, boxes                                                        # the search succeeds here: the groups drew boxes of their own
    if (H, W) == (224, 384):
        assert boxes == {(0, 42, 224, 299)}                                                  # ten failed attempts: the centre-crop fallback


def _blur_restated(x_u8, sigma):
    """GaussianBlur((5, 9)) of the contract in fp32 on the CPU: reflect padding, 9 x 5 product kernel, round half to even"""
    import torch.nn.functional as F
    from safevla_amd.preproc import gaussian_weights
    k = torch.tensor(gaussian_weights(9, sigma))[:, None] * torch.tensor(gaussian_weights(5, sigma))[None, :]
    xp = F.pad(x_u8.cpu().float().permute(0, 3, 1, 2), (2, 2, 4, 4), mode="reflect")
    return F.conv2d(xp, k[None, None].expand(3, 1, 9, 5).contiguous(), groups=3).round().clamp(0, 255).permute(0, 2, 3, 1).to(U8)


def test_posterize_masks_below_seven_bits():
    """factors 1 / 1 / 1 / 0, sigma 0.1, whole-frame box, no sharpness: every stage but posterize returns its input (the off-centre blur weights are below 2e-22 and
    vanish under the centre term in fp32; the restatement of the blur says the same).  Four groups hold the SAME frames with masks 0xFF, 0xFC, 0xF8, 0xF0."""
    from safevla_amd.preproc import RandomAugmentCall, apply_random_augment_u8
    L, H, W = 2, 24, 40
    one = torch.randint(0, 256, (L, H, W, 3), generator=torch.Generator().manual_seed(5), dtype=U8)
    ident = RandomAugmentCall((0, 1, 2, 3), 1.0, 1.0, 1.0, 0.0, 0.1, (0, 0, H, W), 0xFF, False)
    masks = [0xFF, 0xFC, 0xF8, 0xF0]
    out = apply_random_augment_u8(one.repeat(4, 1, 1, 1).cuda(), [ident._replace(post_mask=m) for m in masks], L).cpu().view(4, L, H, W, 3)
    assert torch.equal(_blur_restated(one, 0.1), one)
    assert torch.equal(out[0], _blur_restated(one, 0.1))
    for k, m in enumerate(masks):
        assert torch.equal(out[k], out[0] & m), f"mask {m:#x}"
        assert k == 0 or not torch.equal(out[k], out[k - 1])


def test_one_group_equals_the_single_transform_launches():
    from safevla_amd.preproc import apply_augment_u8, apply_random_augment_u8
    x, calls, _, _ = case(SHAPES[1])
    for c in calls:
        assert torch.equal(apply_random_augment_u8(x, [c], x.shape[0]), apply_augment_u8(x, c.as_augment_call()))


def test_groups_without_contrast_and_with_shorter_orders():
    """The sampler always draws all four operations, but the table takes any order of up to four: a group without contrast needs no gray mean (its blocks of the
    first launch return at once, its partial sums stay unwritten and unread), a group may hold fewer operations or none.  Oracle: the single-transform launches
    (ops.aug_jitter_blur takes shorter orders) on each slice, bit for bit.  The partials buffer is poisoned first, so a group that read its unwritten rows would show."""
    from safevla_amd import ops
    from safevla_amd.preproc import gaussian_weights
    L, H, W = 2, 24, 40
    # (operations, factors, sigma, box, post_mask, sharpen): no contrast; contrast alone; nothing but the blur; contrast second of three; hue alone
    groups = [((0, 2, 3), (1.21, 0.87, 0.031), 0.9, (1, 3, 22, 35), 0xFE, True),
              ((1,), (1.33,), 1.4, (0, 0, 24, 40), 0xFF, False),
              ((), (), 0.6, (2, 0, 21, 39), 0xFC, True),
              ((2, 1, 0), (1.13, 0.71, 0.93), 1.1, (0, 0, 24, 40), 0xFF, True),
              ((3,), (-0.043,), 0.3, (1, 1, 20, 30), 0xFE, False)]
    G = len(groups)
    x = torch.randint(0, 256, (G * L, H, W, 3), generator=torch.Generator().manual_seed(77), dtype=U8).cuda()
    table = ops.AugTable([(o, f, gaussian_weights(5, sg), gaussian_weights(9, sg), box, m, sh) for o, f, sg, box, m, sh in groups], x.device)
    assert [t.nops_before_contrast for t in table.host] == [-1, 0, -1, 1, -1]
    part = ops.aug_gray_partials_grouped(x, table, L)
    ref_part = ops.aug_gray_partials(x[6:8].contiguous(), (2,), (1.13,))                      # group 3: the sums are taken after the one operation before contrast
    assert torch.equal(part[6:8], ref_part) and torch.equal(part[2:4], ops.aug_gray_partials(x[2:4].contiguous()))
    poisoned = part.clone()
    for k in (0, 2, 4):
        poisoned[k * L:(k + 1) * L] = 1 << 60                                                 # the rows the first launch left unwritten
    got = ops.aug_resize_post_sharp_grouped(ops.aug_jitter_blur_grouped(x, table, L, poisoned), table, L)
    for k, (o, f, sg, box, m, sh) in enumerate(groups):
        xs = x[k * L:(k + 1) * L].contiguous()
        p = ops.aug_gray_partials(xs, o[:o.index(1)], f[:o.index(1)]) if 1 in o else None
        y = ops.aug_jitter_blur(xs, o, f, p, gaussian_weights(5, sg), gaussian_weights(9, sg))
        if m in (0xFF, 0xFE):
            want = ops.aug_resize_post_sharp(y, box, m == 0xFE, sh)
        else:                                                                                 # the old launches know 0xFE only: resize, mask on the host, then sharpness
            want = ops.aug_resize_post_sharp(ops.aug_resize_post_sharp(y, box) & m, sharpen=sh)
        assert torch.equal(got[k * L:(k + 1) * L], want), f"group {k}: {o}"


def test_siglip_preprocessor_random_per_call():
    """SigLIPDataAugmentationPreprocessor(random_per_call=True), the reference's online SigLIP class: every augment_u8 / process draws one call of the random list at
    the resized geometry and applies it to the whole batch as one group"""
    from safevla_amd import ops
    from safevla_amd.preproc import SIGLIP_RGB_MEANS, SIGLIP_RGB_STDS, SigLIPDataAugmentationPreprocessor, apply_random_augment_u8, sample_random_augment_call
    x = torch.randint(0, 256, (3, 224, 384, 3), generator=torch.Generator().manual_seed(8), dtype=U8).cuda()
    pre = SigLIPDataAugmentationPreprocessor("rgb", "aug", use_augmentation=True, random_per_call=True, generator=torch.Generator().manual_seed(21))
    g = torch.Generator().manual_seed(21)
    c1, c2 = sample_random_augment_call(256, 256, g), sample_random_augment_call(256, 256, g)
    r = ops.resize_bicubic_aa_u8(x, (256, 256))
    a = pre.augment_u8(x)
    assert pre.last_random_call == c1 and tuple(a.shape) == (3, 256, 256, 3) and torch.equal(a, apply_random_augment_u8(r, [c1], 3))
    b = pre.process({"rgb": x})
    assert pre.last_random_call == c2 and c2 != c1, "the second call did not draw anew"
    assert torch.equal(b, ops.normalize_u8(apply_random_augment_u8(r, [c2], 3), SIGLIP_RGB_MEANS, SIGLIP_RGB_STDS))
    out = torch.empty_like(r)
    pre.generator = torch.Generator().manual_seed(21)
    assert pre.augment_u8(r, out=out) is out and torch.equal(out, a)                          # frames that already are 256 x 256: no resize, the same draw
    # the default is the sampled-specific transform of the schedule, as before
    assert SigLIPDataAugmentationPreprocessor("rgb", "aug", use_augmentation=True).random_per_call is False


def test_repeatable_and_groups_permute():
    from safevla_amd.preproc import apply_random_augment_u8
    shape = SHAPES[0]
    G, L, H, W = shape
    x, calls, got, _ = case(shape)
    assert torch.equal(apply_random_augment_u8(x, calls, L), got), "two runs differ"
    perm = [2, 0, 1]
    xp = x.view(G, L, H, W, 3)[perm].reshape(G * L, H, W, 3).contiguous()
    gp = apply_random_augment_u8(xp, [calls[p] for p in perm], L)
    assert torch.equal(gp.view(G, L, H, W, 3), got.view(G, L, H, W, 3)[perm]), "permuting the groups does not permute the output"
    out = torch.empty_like(x)
    assert apply_random_augment_u8(x, calls, L, out=out) is out and torch.equal(out, got)


def test_refused_tables_launch_nothing():
    from safevla_amd import ops
    from safevla_amd._lib import SvlaError
    from safevla_amd.preproc import RandomAugmentCall, apply_random_augment_u8, gaussian_weights
    H = W = 16
    x = torch.randint(0, 256, (4, H, W, 3), generator=torch.Generator().manual_seed(9), dtype=U8).cuda()
    ok = RandomAugmentCall((0, 1, 2, 3), 1.1, 0.9, 1.05, 0.01, 0.8, (1, 1, 14, 14), 0xFE, True)

    def refused(calls, group_len):
        out = torch.full_like(x, 77)
        with pytest.raises(SvlaError):
            apply_random_augment_u8(x, calls, group_len, out=out)
        torch.cuda.synchronize()
        assert bool((out == 77).all()), "a refused application wrote to its output"

    for box in ((0, 0, 17, 16), (0, 1, 16, 16), (-1, 0, 8, 8), (4, 4, 0, 8), (10, 10, 8, 8)):
        refused([ok, ok._replace(box=box)], 2)                                     # a box outside the image in group 1 only
    for mask in (0x7F, 0xE0, 0x00, 0x1FE):
        refused([ok, ok._replace(post_mask=mask)], 2)
    refused([ok], 3)                                                               # N % group_len != 0
    # each of the three entries refuses on its own (the application stops at the first): the last launch with a bad table leaves its output alone too
    bad = ok._replace(box=(0, 0, 17, 16))
    table = ops.AugTable([(c.order, [c.factor(o) for o in c.order], gaussian_weights(5, c.sigma), gaussian_weights(9, c.sigma), c.box, c.post_mask, c.sharpen)
                          for c in (ok, bad)], x.device)
    out = torch.full_like(x, 77)
    with pytest.raises(SvlaError):
        ops.aug_resize_post_sharp_grouped(x, table, 2, out=out)
    with pytest.raises(SvlaError):
        ops.aug_jitter_blur_grouped(x, table, 2, torch.zeros(4, ops.AUG_NPART, dtype=torch.int64, device=x.device), out=out)
    torch.cuda.synchronize()
    assert bool((out == 77).all())
    for shape in ((2, 4, 16, 3), (2, 16, 2, 3)):                                   # H < 5, W < 3
        small = torch.zeros(shape, dtype=U8, device="cuda")
        with pytest.raises(SvlaError):
            apply_random_augment_u8(small, [ok._replace(box=(0, 0, 1, 1))], 2)
    with pytest.raises(ValueError):
        apply_random_augment_u8(x, [ok], 2)                                        # two groups, one table entry: refused by the wrapper
    assert torch.equal(apply_random_augment_u8(x, [ok, ok], 2), apply_random_augment_u8(x, [ok], 4))      # and the legal table is served
