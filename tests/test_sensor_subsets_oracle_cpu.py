"""The sensor-subset restatements of tests/helpers/sensor_subsets.py against outputs of the reference itself (tests/golden/s1_rl_nav.npz,
s2_il_cameras.npz, s3_il_nav_last.npz, made by tests/golden/make_golden_sensors.py), at the tolerances tests/test_oracle_golden.py uses for G5 / G8;
and the name manifests of the reduced sets: exactly the reference's names."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import sensor_subsets as S      # noqa: E402

from oracle.detfill import fill_state_dict, grad_probe      # noqa: E402
from safevla_amd.text import GoalTokenizer      # noqa: E402


@pytest.fixture(scope="module")
def nav_tower():
    torch.manual_seed(0)
    m = S.SubsetTower(GoalTokenizer(), max_steps=500, max_batch=4).eval()
    fill_state_dict(m, seed=7)
    return m


def test_navigation_only_tower_names_equal_the_reference(nav_tower):
    want = S.manifest("state_dict_manifest_rl_nav.txt")
    have = {k: str(tuple(v.shape)) for k, v in nav_tower.state_dict().items()}
    assert have == want
    full = S.manifest("state_dict_manifest.txt")
    gone = {k for k in full if not k.startswith(("critic_tsfm.", "c_critic_tsfm.")) and k not in want}      # the actor tower's names of the full set
    assert gone == {"visual_encoder.visual_sensor_token_raw_manipulation_camera", "object_in_hand_embed.weight"}


def test_navigation_only_update_pass_vs_reference(nav_tower):
    g, upd, _ = S.load_rl_nav()
    obs = S.to_torch(upd)
    for p in nav_tower.parameters():
        p.grad = None
    logits, values, _ = nav_tower.tower_forward(obs, torch.from_numpy(g["prev_actions"]), torch.from_numpy(g["masks"]))
    lsm = torch.log_softmax(logits, -1)
    np.testing.assert_allclose(lsm.detach().numpy(), g["logits"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(values.detach().numpy(), g["values"], rtol=1e-4, atol=2e-5)
    ((lsm * torch.from_numpy(g["w_logits"])).sum() + (values * torch.from_numpy(g["w_values"])).sum()).backward()
    named = dict(nav_tower.named_parameters())
    assert len(g["grad_names"]) == 84
    for n in g["grad_names"]:
        nrm, prj = grad_probe(str(n), named[str(n)].grad)
        want = g["gp:" + str(n)]
        np.testing.assert_allclose([nrm, prj], want, rtol=2e-3, atol=1e-5 + 1e-4 * want[0], err_msg=str(n))
    have = {n for n, p in named.items() if p.grad is not None and float(p.grad.abs().sum()) > 0}
    assert have == {str(n) for n in g["grad_names"]}


def test_navigation_only_acting_steps_vs_reference(nav_tower):
    g, _, act = S.load_rl_nav()
    obs = S.to_torch(act)
    pa, mk = torch.from_numpy(g["act:prev_actions"]), torch.from_numpy(g["act:masks"])
    nav_tower.time_step_counter = 0
    lg, vs = [], []
    with torch.no_grad():
        for t in range(pa.shape[0]):
            l, v, _ = nav_tower.tower_forward({k: x[t:t + 1] for k, x in obs.items()}, pa[t:t + 1], mk[t:t + 1])
            lg.append(torch.log_softmax(l, -1)); vs.append(v)
    np.testing.assert_allclose(torch.cat(lg).numpy(), g["act:logits"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(torch.cat(vs).numpy(), g["act:values"], rtol=1e-4, atol=2e-5)
    assert g["act:logits"].shape == (7, 4, 20)


@pytest.mark.parametrize("tag", ["s2_il_cameras", "s3_il_nav_last"])
def test_il_sensor_subsets_vs_reference(tag):
    g, sensors, batch = S.load_il(tag)
    m = S.SubsetEarlyFusion(sensors).eval()
    want = S.manifest(f"state_dict_manifest_{tag}.txt")
    have = {k: str(tuple(v.shape)) for k, v in m.state_dict().items()}
    assert have == want
    full = set(S.manifest("state_dict_manifest_il.txt"))
    assert full - set(want) == {"visual_encoder.visual_sensor_token_" + c for c in ("raw_navigation_camera", "raw_manipulation_camera") if c not in sensors} | \
        {n for s, n in (("last_actions", "last_actions_embed.weight"), ("an_object_is_in_hand", "object_in_hand_embed.weight")) if s not in sensors}
    fill_state_dict(m, seed=7, share_t5=False)
    out = m(S.to_torch(batch))
    out["loss"].backward()
    assert np.allclose(out["actions_logits"].detach().numpy(), g["logits"], rtol=2e-4, atol=2e-4)
    assert abs(out["loss"].item() - float(g["loss"])) < 1e-5
    n = 0
    for name, p in m.named_parameters():
        if "gp:" + name in g:
            got = np.array(grad_probe(name, p.grad))
            assert np.allclose(got, g["gp:" + name], rtol=2e-3, atol=1e-6), (name, got, g["gp:" + name])
            n += 1
    assert n == sum(k.startswith("gp:") for k in g) == 82
