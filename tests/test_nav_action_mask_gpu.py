"""Navigation-only action mask (``SafeDinoLLAMATxNavActorCriticSeparate.mask_non_nav_actions``; dinov2_vits_tsfm_base.py:272-289 sets the actor bias of the 13
non-navigation actions to -999999): the masked actions have probability exactly 0, are never sampled, and the fused ``SafePPOLogGrad`` -- entropy term
included -- stays finite with zero gradient on the masked logits (no NaN from 0 * (-1e6))."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAV_IDS = [0, 1, 2, 3, 4, 6, 7]          # m, r, l, b, end, ls, rs of agent.ALL_STRETCH_ACTIONS
MASKED = [i for i in range(20) if i not in NAV_IDS]


@pytest.fixture(scope="module")
def masked_model():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from safevla_amd.model import SafeDinoLLAMATxNavActorCriticSeparate

    torch.manual_seed(3)
    m = SafeDinoLLAMATxNavActorCriticSeparate(device=DEV, full_sensor=False).eval()
    with torch.no_grad():
        m.actor.linear.weight.mul_(30.0)          # (the 0.01-gain initialisation gives near-uniform policies: spread the navigation logits)
    idx = m.mask_non_nav_actions()
    assert idx == MASKED and len(idx) == 13
    return m


def _obs(T, B, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    ids = torch.randint(3, 32000, (T, B, 6), device=DEV, generator=g)
    ids[..., -1] = 1
    ids[:, :] = ids[:1]          # one goal per env column
    obs = {"dino_tokens": torch.randn(T, B, 1, 84, 384, device=DEV, generator=g).to(torch.bfloat16), "goal_token_ids": ids,
           "time_step": torch.arange(T, device=DEV)[:, None].expand(T, B).contiguous(), "traj_index": torch.zeros(T, B, dtype=torch.int64, device=DEV)}
    pa = torch.randint(0, 20, (T, B), device=DEV, generator=g)
    mk = torch.ones(T, B, 1, device=DEV)
    mk[0] = 0
    return obs, pa, mk


def test_bias_and_probabilities_of_masked_actions(masked_model):
    m = masked_model
    b = m.actor.linear.bias.detach().cpu()
    assert (b[MASKED] == -999999).all() and (b[NAV_IDS] == 0).all()
    assert (m.critic_tsfm.actor.linear.bias == 0).all()                   # the actor tower only, as the reference (model.actor.linear.bias)
    obs, pa, mk = _obs(4, 2, seed=1)
    with torch.no_grad():
        out, _ = m(obs, None, pa, mk)
    d = out.distributions
    assert torch.isfinite(d.logits).all() and (d.probs[..., MASKED] == 0).all()
    assert torch.allclose(d.probs[..., NAV_IDS].sum(-1), torch.ones(4, 2, device=DEV), atol=1e-5)
    ent = d.entropy()
    assert torch.isfinite(ent).all() and (ent > 0).all() and (ent <= np.log(7) + 1e-5).all()
    assert all(int(a) in NAV_IDS for a in d.mode().reshape(-1))


def test_sampled_actions_are_navigation_actions(masked_model):
    m = masked_model
    for t in m.towers:
        t.time_step_counter, t._kv = 0, None
    obs, pa, mk = _obs(1, 4, seed=2)
    gen = torch.Generator(device=DEV).manual_seed(7)
    drawn = []
    with torch.no_grad():
        out, _ = m(obs, None, pa, mk)                                     # one acting step x 4 envs ...
        for _ in range(128):                                              # ... 128 draws each: 512 sampled actions
            drawn.append(out.distributions.sample(generator=gen).reshape(-1))
    drawn = torch.cat(drawn).cpu().numpy()
    assert drawn.shape == (512,) and set(drawn.tolist()) <= set(NAV_IDS)
    assert len(set(drawn.tolist())) > 1
    for t in m.towers:
        t.time_step_counter, t._kv = 0, None


def test_safe_ppo_loss_backward_is_finite_with_zero_gradient_on_masked_logits(masked_model):
    from safevla_amd.losses import SafePPOLogGrad

    m = masked_model
    T, B = 4, 2
    obs, pa, mk = _obs(T, B, seed=3)
    rs = np.random.RandomState(4)
    d = lambda a: torch.from_numpy(a).to(DEV)
    batch = {"actions": d(rs.choice(NAV_IDS, size=(T, B)).astype(np.int64)), "old_action_log_probs": d((-2.0 + 0.3 * rs.standard_normal((T, B))).astype(np.float32)),
             "adv_targ": d(rs.standard_normal((T, B, 1)).astype(np.float32)), "c_adv_targ": d(rs.standard_normal((T, B, 1)).astype(np.float32)),
             "returns": d(rs.standard_normal((T, B, 1)).astype(np.float32)), "values": d(rs.standard_normal((T, B, 1)).astype(np.float32))}
    m.zero_grad()
    aco, _ = m(obs, None, pa, mk)
    raw = aco.distributions.raw_logits
    raw.retain_grad()
    assert (raw[..., MASKED] < -9e5).all()
    total, info = SafePPOLogGrad(0.1, 0.5, 0.01, use_clipped_value_loss=False, normalize_advantage=False).loss(0, batch, aco, lagrangian_multiplier=torch.tensor(0.37))
    total.backward()
    assert np.isfinite(float(total.detach())) and all(np.isfinite(info[k]) for k in ("ppo_total", "value", "action", "entropy")), info
    assert torch.isfinite(raw.grad).all() and (raw.grad[..., MASKED] == 0).all() and float(raw.grad[..., NAV_IDS].abs().sum()) > 0
    assert torch.isfinite(m.arena.flat_g).all()
    gb = m.g(m.actor.linear.bias)
    assert (gb[MASKED] == 0).all() and float(gb[NAV_IDS].abs().sum()) > 0
    # the entropy term the loss reports (mean of -H) is the 7-way entropy of the navigation actions: the masked ones contribute exactly nothing
    p = torch.softmax(raw.detach()[..., NAV_IDS].double(), -1)
    assert abs(info["entropy"] - float((p * p.log()).sum(-1).mean())) < 1e-5
