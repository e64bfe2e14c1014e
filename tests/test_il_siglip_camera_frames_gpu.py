"""The SigLIP imitation-learning presets from camera-sized frames: ``siglip_base_3`` (the preset the reference's evaluation scripts load) takes 224 x 384 uint8
frames through the resize of preprocessors.py:35-43 (csrc/resize.hip) in front of its frozen 256 x 256 trunk -- ``forward(batch)`` and the online agent's
``get_action`` -- and 256 x 256 frames exactly as before."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAV, MANIP = "raw_navigation_camera", "raw_manipulation_camera"


def _batch(nav, man, T):
    ids = torch.ones(1, 64, dtype=torch.int64)
    ids[0, :6] = torch.tensor([917, 4033, 88, 21, 305, 12])
    return {NAV: nav, MANIP: man, "time_ids": torch.arange(T, device=DEV)[None], "an_object_is_in_hand": torch.zeros(1, T, dtype=torch.int64, device=DEV),
            "last_actions": torch.tensor([[20] + [3] * (T - 1)], device=DEV), "goals": ids.to(DEV)}


@pytest.fixture(scope="module")
def model():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from oracle.detfill import fill_state_dict
    from safevla_amd.il import EarlyFusionCnnTransformer
    m = EarlyFusionCnnTransformer.build_model("siglip_base_3", device=DEV)
    fill_state_dict(m, seed=23, share_t5=False)
    m.sync_weights()
    m.eval()
    return m


def test_forward_on_camera_frames_equals_forward_on_resized_frames(model):
    from safevla_amd import ops
    g = torch.Generator().manual_seed(31)
    T = 2
    nav, man = (torch.randint(0, 256, (1, T, 224, 384, 3), generator=g, dtype=torch.uint8).to(DEV) for _ in range(2))
    rs = lambda x: ops.resize_bicubic_aa_u8(x.reshape(T, 224, 384, 3), (256, 256)).reshape(1, T, 256, 256, 3)
    with torch.no_grad():
        got = model(_batch(nav, man, T))["actions_logits"]
        want = model(_batch(rs(nav), rs(man), T))["actions_logits"]
    assert tuple(got.shape) == (1, T, 20) and bool(torch.isfinite(got).all())
    assert torch.equal(got, want)


def test_256_frames_take_the_route_they_took_before(model):
    """the model's own preprocessor (a SigLIPPreprocessor behind the resizing front) against a bare SigLIPPreprocessor passed explicitly -- the route before the
    front existed -- with the same trunk weights"""
    from oracle.detfill import fill_state_dict
    from safevla_amd.il import EarlyFusionCnnTransformer
    from safevla_amd.preproc import SigLIPPreprocessor
    g = torch.Generator().manual_seed(32)
    T = 2
    nav, man = (torch.randint(0, 256, (1, T, 256, 256, 3), generator=g, dtype=torch.uint8).to(DEV) for _ in range(2))
    with torch.no_grad():
        got = model(_batch(nav, man, T))["actions_logits"]
    bare = SigLIPPreprocessor(NAV, NAV, device=DEV)
    bare.vit.load_state_dict(model.image_preprocessor.vit.state_dict())
    m2 = EarlyFusionCnnTransformer(device=DEV, image_preprocessor=bare, dino_dim=768, text_encoder="SigLIPBase")
    fill_state_dict(m2, seed=23, share_t5=False)      # the fixture's weights
    m2.sync_weights()
    m2.eval()
    with torch.no_grad():
        want = m2(_batch(nav, man, T))["actions_logits"]
    assert m2.image_preprocessor is bare and not bare.augmenters
    assert torch.equal(got, want)


def test_agent_acts_on_camera_frames():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from safevla_amd.il import EarlyFusionCnnTransformer
    agent = EarlyFusionCnnTransformer.build_agent("siglip_base_3", device=DEV, tokenizer=None)
    rs = np.random.RandomState(5)
    goal = torch.ones(1, 64, dtype=torch.int64)
    goal[0, :5] = torch.tensor([44, 1810, 9, 2177, 63])
    for t in range(3):
        obs = {NAV: rs.randint(0, 256, (224, 384, 3)).astype(np.uint8), MANIP: rs.randint(0, 256, (224, 384, 3)).astype(np.uint8), "an_object_is_in_hand": [0]}
        a, p = agent.get_action(obs, goal)
        assert a in agent.get_action_list() and tuple(p.shape) == (20,) and bool(torch.isfinite(p).all()) and abs(float(p.sum()) - 1.0) < 1e-4
    assert agent.curr_t == 3
