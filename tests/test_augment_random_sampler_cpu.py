"""Host side of the per-trajectory random v2 augmentation (preproc.sample_random_augment_call): the per-call draws of the reference's random list
(utils/transformation_util.py:12-28 as the IL Preprocessor applies it, preprocessors.py:86-118), on a torch generator, in Compose order.  No device needed.

torchvision is not installed, so the draw sequence is restated here by hand and the sampler must consume exactly it: randperm(4); brightness, contrast,
saturation, hue; sigma; per crop attempt a scale and a log-ratio (top and left on success); four posterize coins; one sharpness coin."""
import itertools
import math

import torch

from safevla_amd.preproc import (AUG_CONTRAST, CROP_RATIO, RandomAugmentCall, crop_fallback_box, gaussian_weights, posterize_mask,
                                 sample_random_augment_call)


def _u(g, lo, hi):
    return torch.empty(1).uniform_(lo, hi, generator=g).item()


def _replay(H, W, g):
    """the sequence of the module docstring, written out; returns (call fields, crop attempts made, the scale of the attempt that fitted or None)"""
    order = tuple(torch.randperm(4, generator=g).tolist())
    b, c, s, h = _u(g, 0.6, 1.4), _u(g, 0.6, 1.4), _u(g, 0.8, 1.2), _u(g, -0.05, 0.05)
    sigma = _u(g, 0.1, 2.0)
    box, attempts, scale = None, 0, None
    for _ in range(10):
        attempts += 1
        sc = _u(g, 0.9, 1.0)
        ar = math.exp(_u(g, math.log(CROP_RATIO[0]), math.log(CROP_RATIO[1])))
        w, hh = int(round(math.sqrt(H * W * sc * ar))), int(round(math.sqrt(H * W * sc / ar)))
        if 0 < w <= W and 0 < hh <= H:
            top = int(torch.randint(0, H - hh + 1, (1,), generator=g).item())
            left = int(torch.randint(0, W - w + 1, (1,), generator=g).item())
            box, scale = (top, left, hh, w), sc
            break
    if box is None:
        box = crop_fallback_box(H, W)
    coins = [torch.rand(1, generator=g).item() < 0.2 for _ in range(4)]
    sharpen = torch.rand(1, generator=g).item() < 0.5
    return RandomAugmentCall(order, b, c, s, h, sigma, box, posterize_mask(coins), bool(sharpen)), attempts, scale


def test_same_seed_same_calls():
    a = [sample_random_augment_call(224, 384, torch.Generator().manual_seed(7)) for _ in range(2)]
    assert a[0] == a[1]
    g1, g2 = torch.Generator().manual_seed(7), torch.Generator().manual_seed(7)
    s1 = [sample_random_augment_call(64, 64, g1) for _ in range(5)]
    s2 = [sample_random_augment_call(64, 64, g2) for _ in range(5)]
    assert s1 == s2 and len(set(s1)) == 5                      # a stream of calls repeats under its seed, and the calls of a stream differ
    assert sample_random_augment_call(64, 64, torch.Generator().manual_seed(8)) != s1[0]


def test_camera_frame_consumes_all_twenty_crop_draws_and_falls_back():
    """224 x 384: a box of area >= 0.9 * 86016 with ratio <= 4/3 is at least round(sqrt(0.9 * 86016 * 3/4)) = 241 rows high, so all ten attempts fail -- and each
    still consumes its scale and its ratio.  The generator ends exactly where the hand-replayed sequence ends, so the NEXT call draws the same on both."""
    for seed in range(5):
        g1, g2 = torch.Generator().manual_seed(seed), torch.Generator().manual_seed(seed)
        call = sample_random_augment_call(224, 384, g1)
        ref, attempts, _ = _replay(224, 384, g2)
        assert attempts == 10 and call.box == (0, 42, 224, 299)
        assert call == ref
        assert torch.equal(g1.get_state(), g2.get_state())
    # the count itself: 1 randperm + 4 factors + 1 sigma + 20 crop draws + 4 + 1 coins.  Skipping the 20 crop draws lands elsewhere.
    g1, g3 = torch.Generator().manual_seed(0), torch.Generator().manual_seed(0)
    sample_random_augment_call(224, 384, g1)
    torch.randperm(4, generator=g3)
    for _ in range(5 + 20 + 5):
        torch.rand(1, generator=g3)                            # uniform_ and rand both take one draw of the stream per element
    assert torch.equal(torch.rand(1, generator=g1), torch.rand(1, generator=g3))


def test_square_frame_box_inside_with_drawn_scale():
    seen = set()
    for seed in range(50):
        g1, g2 = torch.Generator().manual_seed(seed), torch.Generator().manual_seed(seed)
        call = sample_random_augment_call(64, 64, g1)
        ref, attempts, scale = _replay(64, 64, g2)
        assert call == ref and torch.equal(g1.get_state(), g2.get_state())
        top, left, bh, bw = call.box
        assert 0 <= top and 0 <= left and bh >= 1 and bw >= 1 and top + bh <= 64 and left + bw <= 64
        if scale is not None:                                   # an attempt fitted: h, w are sqrt(area / r), sqrt(area r) rounded -> |h w - area| <= (h + w) / 2 + 1/4
            assert 0.9 <= scale <= 1.0
            assert abs(bh * bw - scale * 64 * 64) <= 0.5 * (bh + bw) + 0.25
        else:
            assert call.box == (0, 0, 64, 64)
        seen.add(call.box)
    assert len(seen) > 10                                       # the box moves from call to call


def test_posterize_mask_is_the_and_of_the_chain():
    masks = {7: 0xFE, 6: 0xFC, 5: 0xF8, 4: 0xF0}
    for coins in itertools.product((False, True), repeat=4):
        chain = 0xFF
        for bits, c in zip((7, 6, 5, 4), coins):
            if c:
                chain &= masks[bits]
        assert posterize_mask(coins) == chain, coins
    assert posterize_mask((False,) * 4) == 0xFF and posterize_mask((True, False, False, False)) == 0xFE and posterize_mask((True, False, True, False)) == 0xF8


def test_ranges_over_a_thousand_calls():
    g = torch.Generator().manual_seed(123)
    calls = [sample_random_augment_call(64, 64, g) for _ in range(1000)]
    for c in calls:
        assert sorted(c.order) == [0, 1, 2, 3]
        assert 0.6 <= c.brightness <= 1.4 and 0.6 <= c.contrast <= 1.4 and 0.8 <= c.saturation <= 1.2 and -0.05 <= c.hue <= 0.05
        assert 0.1 <= c.sigma <= 2.0
        assert c.post_mask in (0xFF, 0xFE, 0xFC, 0xF8, 0xF0) and isinstance(c.sharpen, bool)
        assert c.factor(AUG_CONTRAST) == c.contrast
        assert abs(sum(gaussian_weights(5, c.sigma)) - 1) < 1e-5
    # every value of the discrete draws turns up: 24 orders, 5 masks (P(no coin) = 0.41, P(4 bits) = 0.2), both sharpness outcomes (P = 0.5)
    assert len({c.order for c in calls}) == 24
    assert {c.post_mask for c in calls} == {0xFF, 0xFE, 0xFC, 0xF8, 0xF0}
    n_sharp = sum(c.sharpen for c in calls)
    assert 400 < n_sharp < 600                                  # 500 +- 6 sigma (sigma = 15.8)
    n_plain = sum(c.post_mask == 0xFF for c in calls)
    assert 320 < n_plain < 500                                  # 0.8^4 = 0.4096 -> 410 +- 6 sigma (sigma = 15.6)


def test_as_augment_call_keeps_the_transform():
    c = sample_random_augment_call(64, 64, torch.Generator().manual_seed(3))._replace(post_mask=0xFE, sharpen=True)
    a = c.as_augment_call()
    assert a.order == c.order and a.box == c.box and a.params.posterize and a.params.sharpness == 1 and a.params.sigma == c.sigma
    assert [a.params.factor(o) for o in range(4)] == [c.factor(o) for o in range(4)]
    assert not c._replace(post_mask=0xFF).as_augment_call().params.posterize
