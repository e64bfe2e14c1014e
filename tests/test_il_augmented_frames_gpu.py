"""Imitation-learning training from raw frames with the reference's frame augmentation (``data_augmentation=True``: the random v2 list, one newly drawn
transform per trajectory and camera; preprocessors.py:86-118): ``forward(batch)`` passes each camera's uint8 frames through its augmenter in front of the
frozen trunk.  Checked against the pieces: the same seeded draws applied with ``preproc.apply_random_augment_u8`` and fed to the un-augmented forward."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAV, MANIP = "raw_navigation_camera", "raw_manipulation_camera"


def _seed(model, s):
    for cam, a in enumerate(model.augmenters):
        a.generator = torch.Generator().manual_seed(s + cam)


def _calls(H, W, s, B):
    """what _seed(model, s) makes the two cameras draw for a batch of B trajectories"""
    from safevla_amd.preproc import sample_random_augment_call
    out = []
    for cam in range(2):
        g = torch.Generator().manual_seed(s + cam)
        out.append([sample_random_augment_call(H, W, g) for _ in range(B)])
    return out


def _batch(nav, man, goals):
    B, T = nav.shape[:2]
    return {NAV: nav, MANIP: man, "time_ids": torch.arange(T, device=DEV)[None].expand(B, T).contiguous(),
            "an_object_is_in_hand": torch.zeros(B, T, dtype=torch.int64, device=DEV),
            "last_actions": torch.tensor([[20] + [3] * (T - 1)] * B, device=DEV), "goals": goals}


@pytest.fixture(scope="module")
def small_pair():
    """small_3 twice with the same weights and ONE frozen trunk: built with and without data_augmentation"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from oracle.detfill import fill_state_dict
    from safevla_amd.il import EarlyFusionCnnTransformer
    ms = []
    for aug in (False, True):
        m = EarlyFusionCnnTransformer.build_model("small_3", data_augmentation=aug, device=DEV)
        fill_state_dict(m, seed=41)
        m.sync_weights()
        m.eval()
        ms.append(m)
    ms[0].image_preprocessor = ms[0]._frozen_image_encoder(NAV, torch.device(DEV))
    ms[1].image_preprocessor = ms[0].image_preprocessor
    B, T = 2, 3
    g = torch.Generator().manual_seed(51)
    nav, man = (torch.randint(0, 256, (B, T, 224, 384, 3), generator=g, dtype=torch.uint8).to(DEV) for _ in range(2))
    ids = torch.randint(3, 32000, (B, 12), generator=g)
    goals = dict(input_ids=ids.to(DEV), attention_mask=torch.ones_like(ids).to(DEV))
    return ms[0], ms[1], nav, man, goals


def test_small_3_forward_augments_each_trajectory_with_its_own_draw(small_pair):
    from safevla_amd.preproc import apply_random_augment_u8
    plain, augd, nav, man, goals = small_pair
    B, T = nav.shape[:2]
    _seed(augd, 77)
    with torch.no_grad():
        got = augd(_batch(nav, man, goals))["actions_logits"]
    calls = _calls(224, 384, 77, B)
    assert [a.last_calls for a in augd.augmenters] == calls and calls[0] != calls[1] and calls[0][0] != calls[0][1]
    aug = [apply_random_augment_u8(x.reshape(B * T, 224, 384, 3), c, T).view(B, T, 224, 384, 3) for x, c in zip((nav, man), calls)]
    with torch.no_grad():
        want = plain(_batch(aug[0], aug[1], goals))["actions_logits"]
        bare = plain(_batch(nav, man, goals))["actions_logits"]
    assert tuple(got.shape) == (B, T, 20) and bool(torch.isfinite(got).all())
    assert torch.equal(got, want)
    assert not torch.equal(got, bare), "the augmentation changed nothing"


def test_default_is_the_forward_without_augmentation(small_pair):
    plain, augd, nav, man, goals = small_pair
    assert plain.data_augmentation is False and not hasattr(plain, "augmenters")
    with torch.no_grad():
        a = plain(_batch(nav, man, goals))["actions_logits"]
        # today's forward, spelled out: prepare without augmentation -> the tower
        from safevla_amd.il import _TowerFn
        b = _TowerFn.apply(plain._anchor, plain, plain.prepare(_batch(nav, man, goals)), True, False)[0].transpose(0, 1)
        # pre-encoded features never meet the augmenters, whatever the flag says
        feats = torch.randn(2, 3, 384, 7, 12, generator=torch.Generator().manual_seed(3)).to(DEV)
        _seed(augd, 5)
        state = [a_.generator.get_state() for a_ in augd.augmenters]
        c = augd(_batch(feats, feats, goals))["actions_logits"]
        d = plain(_batch(feats, feats, goals))["actions_logits"]
    assert torch.equal(a, b) and torch.equal(c, d)
    assert all(torch.equal(s, a_.generator.get_state()) for s, a_ in zip(state, augd.augmenters)), "features consumed augmentation draws"


def test_siglip_base_3_augments_behind_the_resize():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from oracle.detfill import fill_state_dict
    from safevla_amd import ops
    from safevla_amd.il import EarlyFusionCnnTransformer
    from safevla_amd.preproc import apply_random_augment_u8
    m = EarlyFusionCnnTransformer.build_model("siglip_base_3", data_augmentation=True, device=DEV)
    fill_state_dict(m, seed=23, share_t5=False)
    m.sync_weights()
    m.eval()
    assert [a.size for a in m.augmenters] == [(256, 256)] * 2
    B, T = 1, 2
    g = torch.Generator().manual_seed(61)
    nav, man = (torch.randint(0, 256, (B, T, 224, 384, 3), generator=g, dtype=torch.uint8).to(DEV) for _ in range(2))
    ids = torch.ones(1, 64, dtype=torch.int64)
    ids[0, :6] = torch.tensor([917, 4033, 88, 21, 305, 12])
    _seed(m, 88)
    with torch.no_grad():
        got = m(_batch(nav, man, ids.to(DEV)))["actions_logits"]
    calls = _calls(256, 256, 88, B)                                   # drawn at the resized geometry
    assert [a.last_calls for a in m.augmenters] == calls
    aug = [apply_random_augment_u8(ops.resize_bicubic_aa_u8(x.reshape(B * T, 224, 384, 3), (256, 256)), c, T).view(B, T, 256, 256, 3)
           for x, c in zip((nav, man), calls)]
    m.data_augmentation = False
    with torch.no_grad():
        want = m(_batch(aug[0], aug[1], ids.to(DEV)))["actions_logits"]
    assert tuple(got.shape) == (B, T, 20) and bool(torch.isfinite(got).all())
    assert torch.equal(got, want)


def test_train_il_step_with_augmented_raw_frames():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from safevla_amd.il import EarlyFusionCnnTransformer, ILTrainer
    from safevla_amd.train_il import synthetic_batch
    m = EarlyFusionCnnTransformer.build_model("small_3", data_augmentation=True, device=DEV)      # as train_il --raw_frames --data_augmentation builds it
    _seed(m, 4321)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1234)
    batch = synthetic_batch(2, 3, 12, torch.device(DEV), gen, raw_frames=True, feat_dim=m.dino_dim)
    out = ILTrainer(m).training_step(batch)
    assert math.isfinite(out["loss"]) and out["loss"] > 0
    assert all(len(a.last_calls) == 2 for a in m.augmenters)
