"""Reduced sensor sets on the HIP kernels against outputs of the reference itself (tests/golden/make_golden_sensors.py):

  * navigation-only RL towers (``manipulation_rgb_dino_preprocessor_uuid = an_object_is_in_hand_uuid = None``: one camera token, no in-hand embedding, fusion
    sequences of 1 + 84 + L tokens) vs fixture (a) on the bf16 product path and in the fp32 verification mode, at the gates of the full-sensor golden tests
    (test_model_gpu.py: 2e-2 outputs, 4e-2 gradient checksums, 3e-2 acting steps; test_fp32_mode_gpu.py: 1e-4 / 1e-3); the acting steps on the plain, the
    recorded and the tower-grouped path, recorded == grouped bit for bit as test_grouped_gpu.py requires;
  * the imitation-learning model over ``input_sensors`` vs fixtures (b) and (c) at the gates of test_il_gpu.py, the names of ``state_dict()`` per set, the
    single-camera agent;
  * one ``PPOLagEngine.update`` on a navigation-only model vs the CPU restatement (tests/helpers/sensor_subsets.py) at the small engine test's tolerance, and
    the IL -> RL hand-off between models of the same cameras."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import sensor_subsets as S      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAV, MANIP = "raw_navigation_camera", "raw_manipulation_camera"


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-12)


def _nav_model(precision):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from safevla_amd.model import SafeDinoLLAMATxNavActorCriticSeparate

    m = SafeDinoLLAMATxNavActorCriticSeparate(device=DEV, precision=precision, manipulation_rgb_dino_preprocessor_uuid=None, an_object_is_in_hand_uuid=None)
    S.fill_towers_alike(m, seed=7)          # every tower = the reference tower of fixture (a)
    m.sync_weights()
    return m.eval()


@pytest.fixture(scope="module")
def nav16():
    return _nav_model("bf16")


@pytest.fixture(scope="module")
def nav32():
    return _nav_model("fp32")


def test_navigation_only_constructor_and_names(nav16):
    from safevla_amd.model import SafeDinoLLAMATxNavActorCriticSeparate, Tower

    m = nav16
    assert not m.full_sensor and all((t.ncam, t.text_off, t.has_hand, t.has_prev) == (1, 85, False, True) for t in m.towers)
    assert m._camtok.shape == (1, 512) and m.uuids["manip"] is None and m.uuids["hand"] is None
    want = S.manifest("state_dict_manifest_rl_nav.txt")
    have = {k: str(tuple(v.shape)) for k, v in m.state_dict().items()}
    assert have == {p + k: v for p in ("", "critic_tsfm.", "c_critic_tsfm.") for k, v in want.items()}
    # a checkpoint of another sensor set (here: the model's own tensors + the in-hand table): refused by name
    other = dict(m.state_dict())
    other["object_in_hand_embed.weight"] = torch.zeros(3, 512)
    with pytest.raises(RuntimeError, match="object_in_hand_embed.weight"):
        m.load_state_dict(other, strict=True)
    with pytest.raises(ValueError, match="subset"):
        Tower(m.arena, DEV, cameras=("raw_navigation_camera", "raw_navigation_camera"))
    import inspect
    sig = inspect.signature(SafeDinoLLAMATxNavActorCriticSeparate.__init__).parameters
    assert sig["full_sensor"].default is True and sig["manipulation_rgb_dino_preprocessor_uuid"].default == "manipulation_rgb_dinov2" \
        and sig["an_object_is_in_hand_uuid"].default == "an_object_is_in_hand"


def _update_pass(model, prune_last):
    from oracle.detfill import grad_probe
    from safevla_amd.model import _TowerFn

    g, upd, _ = S.load_rl_nav()
    obs = S.to_torch(upd, DEV)
    for t in model.towers:
        t.prune_last = prune_last
    model.zero_grad()
    prep = model.prepare(obs, torch.from_numpy(g["prev_actions"]).to(DEV), torch.from_numpy(g["masks"]).to(DEV))
    assert prep.S == 85 + prep.L and prep.tokens.shape[1] == 1 and prep.hand is None
    logits, values, _ = _TowerFn.apply(model._anchor, model, prep, True, True)          # ONE tower, both heads: the reference tower of the fixture
    lsm = torch.log_softmax(logits, -1)
    ((lsm * torch.from_numpy(g["w_logits"]).to(DEV)).sum() + (values * torch.from_numpy(g["w_values"]).to(DEV)).sum()).backward()
    e_l, e_v = rel(lsm.detach().cpu().numpy(), g["logits"]), rel(values.detach().cpu().numpy(), g["values"])
    named = dict(model.named_parameters())
    worst = []
    for n in g["grad_names"]:
        n = str(n)
        nrm, prj = grad_probe(n, named[n].grad)
        wn, wp = g["gp:" + n]
        worst.append((abs(nrm - wn) / (wn + 1e-12), abs(prj - wp) / (wn + 1e-12), n))
    worst.sort(reverse=True)
    have = {n for n, p in named.items() if not n.startswith(("critic_tsfm.", "c_critic_tsfm.")) and p.grad is not None and float(p.grad.abs().sum()) > 0}
    for t in model.towers:
        t.prune_last = True
    return e_l, e_v, worst, have, {str(n) for n in g["grad_names"]}


@pytest.mark.parametrize("prune_last", [True, False])
def test_navigation_only_update_pass_vs_reference_bf16(nav16, prune_last):
    e_l, e_v, worst, have, want = _update_pass(nav16, prune_last)
    print(f"[nav-only bf16 prune_last={prune_last}] rel-to-max err: logits {e_l:.3e} values {e_v:.3e}; worst grad checksums",
          [(f"{a:.2e}", f"{b:.2e}", n) for a, b, n in worst[:4]])
    assert e_l < 2e-2 and e_v < 2e-2                                    # test_model_gpu.py's forward gate
    bad = [w for w in worst if w[0] > 4e-2 or w[1] > 4e-2]              # ... and its gradient-checksum gate
    assert not bad, bad[:10]
    assert have == want, have ^ want


@pytest.mark.parametrize("prune_last", [True, False])
def test_navigation_only_update_pass_vs_reference_fp32_mode(nav32, prune_last):
    e_l, e_v, worst, have, want = _update_pass(nav32, prune_last)
    print(f"[nav-only fp32 prune_last={prune_last}] rel-to-max err: logits {e_l:.2e} values {e_v:.2e}; worst grad checksum", worst[0])
    assert e_l < 1e-4 and e_v < 1e-4                                    # test_fp32_mode_gpu.py's gates
    assert max(worst[0][0], max(w[1] for w in worst)) < 1e-3, worst[:5]
    assert have == want, have ^ want


def _acting_steps(model, path):
    """7 steps x 4 envs from fresh caches -> (logits, values, c_values) [7, 4, .] and the KV caches; ``path``: plain | recorded | grouped"""
    g, _, act = S.load_rl_nav()
    obs = S.to_torch(act, DEV)
    pa, mk = torch.from_numpy(g["act:prev_actions"]).to(DEV), torch.from_numpy(g["act:masks"]).to(DEV)
    for t in model.towers:
        t.time_step_counter, t._kv = 0, None
    saved = model._acting_graphs, model._acting_backend, model.grouped_towers
    if path == "plain":
        model.enable_acting_graphs(False)
    else:
        model.enable_acting_plans(True)
        model.grouped_towers = path == "grouped"
    lg, vs, cs = [], [], []
    try:
        with torch.no_grad():
            for t in range(pa.shape[0]):
                o, _ = model({k: v[t:t + 1] for k, v in obs.items()}, None, pa[t:t + 1], mk[t:t + 1])
                lg.append(o.distributions.logits.float().clone()); vs.append(o.values.float().clone()); cs.append(o.c_values.float().clone())
        torch.cuda.synchronize()
        kv = [c.clone() for t in model.towers for c in t._kv]
    finally:
        model._acting_graphs, model._acting_backend, model.grouped_towers = saved
        for t in model.towers:
            t.time_step_counter, t._kv = 0, None
    return torch.cat(lg), torch.cat(vs), torch.cat(cs), kv


def test_navigation_only_acting_steps_on_all_three_paths_bf16(nav16):
    from safevla_amd import ops

    g, _, _ = S.load_rl_nav()
    outs = {}
    for path in ("plain", "recorded", "grouped"):
        ops.group_stats()
        outs[path] = _acting_steps(nav16, path)
        stats = ops.group_stats()
        if path == "grouped":
            assert stats[0] > 50 * 4 and stats[1] == 0, stats            # steps 1, 2 and 4 .. 6 replay as grouped launches (step 3 records the shorter goal batch), none singly
        lg, vs, cs, _ = outs[path]
        e = (rel(lg.cpu().numpy(), g["act:logits"]), rel(vs.cpu().numpy(), g["act:values"]), rel(cs.cpu().numpy(), g["act:values"]))
        print(f"[nav-only acting, {path}] rel-to-max err: logits {e[0]:.3e} values {e[1]:.3e} c_values {e[2]:.3e}")
        assert max(e) < 3e-2, (path, e)                                  # test_model_gpu.py::test_acting_path_kv_cache_vs_reference
    # the grouped replay is the recorded steps' kernels in other grids: bit-identical, KV caches included (test_grouped_gpu.py)
    for a, b in zip(outs["grouped"][:3], outs["recorded"][:3]):
        assert torch.equal(a, b), float((a - b).abs().max())
    for a, b in zip(outs["grouped"][3], outs["recorded"][3]):
        assert torch.equal(a, b)
    # recorded vs plain: the same arithmetic over the whole cache window behind the mask (test_model_gpu.py::test_acting_graph_replay_equals_eager_acting)
    for a, b in zip(outs["recorded"][:3], outs["plain"][:3]):
        assert torch.allclose(a, b, rtol=0, atol=2e-2 * max(1.0, b.abs().max().item())), float((a - b).abs().max())


def test_navigation_only_acting_steps_fp32_mode(nav32):
    g, _, _ = S.load_rl_nav()
    lg, vs, cs, _ = _acting_steps(nav32, "plain")
    e = (rel(lg.cpu().numpy(), g["act:logits"]), rel(vs.cpu().numpy(), g["act:values"]), rel(cs.cpu().numpy(), g["act:values"]))
    print(f"[nav-only acting, fp32 mode] rel-to-max err: logits {e[0]:.2e} values {e[1]:.2e} c_values {e[2]:.2e}")
    assert max(e) < 1e-4, e


# ------------------------------------------------------------------------------------------------ imitation learning
@pytest.mark.parametrize("tag", ["s2_il_cameras", "s3_il_nav_last"])
def test_il_input_sensors_vs_reference(tag):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from oracle.detfill import fill_state_dict, grad_probe
    from safevla_amd.il import EarlyFusionCnnTransformer

    g, sensors, batch = S.load_il(tag)
    m = EarlyFusionCnnTransformer.build_model("small_3", sensors, device=DEV)
    assert {k: str(tuple(v.shape)) for k, v in m.state_dict().items()} == S.manifest(f"state_dict_manifest_{tag}.txt")
    assert m.cameras == tuple(c for c in (NAV, MANIP) if c in sensors) and m.has_prev == ("last_actions" in sensors) and not m.has_hand
    fill_state_dict(m, seed=7, share_t5=False)
    m.sync_weights()
    m.eval()
    m.zero_grad()
    out = m(S.to_torch(batch, DEV))
    out["loss"].backward()
    lg = out["actions_logits"].detach().float().cpu().numpy()
    assert lg.shape == g["logits"].shape
    own = dict(m.named_parameters())
    errs = []
    for k in g:
        if k.startswith("gp:"):
            name = k[3:].replace("actor.weight", "actor.linear.weight").replace("actor.bias", "actor.linear.bias")
            errs.append(abs(np.array(grad_probe(k[3:], own[name].grad))[0] - g[k][0]) / (abs(g[k][0]) + 1e-9))
    errs = np.array(errs)
    print(f"[{tag}] logits rel err {rel(lg, g['logits']):.3e}, loss {float(out['loss'].detach()):.5f} vs {float(g['loss']):.5f}; grad checksums median {np.median(errs):.2e} max {errs.max():.2e}")
    assert rel(lg, g["logits"]) < 3e-2                                                                  # the gates of test_il_gpu.py
    assert abs(float(out["loss"].detach()) - float(g["loss"])) < 3e-2 * abs(float(g["loss"]))
    assert len(errs) == 82 and np.median(errs) < 2e-2 and errs.max() < 8e-2, (np.median(errs), errs.max())
    # a checkpoint of the four-sensor set does not fit: strict loading names what differs
    four = {k: torch.zeros([int(x) for x in shp.strip("()").split(",") if x.strip()]) for k, shp in S.manifest("state_dict_manifest_il.txt").items()}
    with pytest.raises(RuntimeError, match="object_in_hand_embed.weight"):
        m.load_state_dict(four, strict=True)


def test_il_default_sensors_keep_their_names_and_unknown_sensors_are_refused():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from safevla_amd.il import EarlyFusionCnnTransformer

    m = EarlyFusionCnnTransformer.build_model("small_3", device=DEV)
    assert {k: str(tuple(v.shape)) for k, v in m.state_dict().items()} == S.manifest("state_dict_manifest_il.txt")
    assert (m.ncam, m.text_off, m.has_hand, m.has_prev) == (2, 169, True, True)
    for bad in ("nav_task_relevant_object_bbox", "relative_arm_location_metadata", "raw_navigation_camera_1"):
        with pytest.raises(ValueError, match="raw_manipulation_camera.*last_actions"):                  # the message lists what is built
            EarlyFusionCnnTransformer.build_model("small_3", [NAV, bad], device=DEV)
    with pytest.raises(ValueError, match="camera"):
        EarlyFusionCnnTransformer.build_model("small_3", ["last_actions"], device=DEV)


def test_il_single_camera_agent_steps_equal_full_sequence_forward():
    """the agent of fixture (c)'s sensor set takes single-camera observations; its steps equal forward(batch) on the window (test_il_gpu.py's agent test)"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from oracle.detfill import fill_state_dict
    from safevla_amd.il import EarlyFusionCnnTransformer

    agent = EarlyFusionCnnTransformer.build_agent("small_3", [NAV, "last_actions"], device=DEV, sampling="greedy")
    m = agent.model
    fill_state_dict(m, seed=17, share_t5=False)
    m.sync_weights()
    m.eval()
    rs = np.random.RandomState(8)
    T = 6
    nav = rs.standard_normal((T, 384, 7, 12)).astype(np.float32)
    goal = dict(input_ids=np.array([[917, 4033, 88, 21, 1]]), attention_mask=np.ones((1, 5), np.int64))
    acts, probs = [], []
    for t in range(T):
        a, p = agent.get_action({NAV: nav[t]}, goal)                                # no manipulation frame, no in-hand observation
        acts.append(agent.get_action_list().index(a)); probs.append(p.float().cpu().numpy())
        assert p.shape == (20,) and abs(float(p.sum()) - 1.0) < 1e-4
    assert agent.curr_t == T and agent.cache["last_actions"] == acts[-1]
    batch = {NAV: torch.from_numpy(nav)[None].to(DEV), "time_ids": torch.arange(T, device=DEV)[None], "last_actions": torch.tensor([[20] + acts[:-1]], device=DEV),
             "goals": {k: torch.as_tensor(v).to(DEV) for k, v in goal.items()}}
    with torch.no_grad():
        ref = torch.softmax(m(batch)["actions_logits"][0].float(), -1).cpu().numpy()
    got = np.stack(probs)
    assert np.abs(got - ref).max() < 2e-2 * max(ref.max(), 1e-3), np.abs(got - ref).max()
    # without "last_actions" the agent keeps no previous action (early_fusion_tsfm_models.py:507-508)
    a2 = EarlyFusionCnnTransformer.build_agent("small_3", [NAV, MANIP], device=DEV)
    a2.get_action({NAV: nav[0], MANIP: nav[1]}, goal)
    assert "last_actions" not in a2.cache and a2.curr_t == 1


# ------------------------------------------------------------------------------------------------ engine, storage, hand-off
def test_engine_update_on_a_navigation_only_model_vs_restatement(nav16):
    from oracle import ref_loss
    from oracle.ref_rollout import RefLagrange, gae_scan
    from safevla_amd.engine import PPOLagConfig, PPOLagEngine
    from safevla_amd.storage import RolloutStorage
    from safevla_amd.text import GoalTokenizer

    from oracle.detfill import fill_state_dict

    model = nav16
    p_alike = model.arena.flat_p.clone()
    try:
        fill_state_dict(model, seed=7)          # three different towers for this test
        model.sync_weights()
        _engine_update_vs_restatement(model, p_alike, ref_loss, RefLagrange, gae_scan, PPOLagConfig, PPOLagEngine, RolloutStorage, GoalTokenizer)
    finally:
        model.arena.flat_p.copy_(p_alike)
        model.sync_weights(frozen=False)


def _engine_update_vs_restatement(model, p_alike, ref_loss, RefLagrange, gae_scan, PPOLagConfig, PPOLagEngine, RolloutStorage, GoalTokenizer):
    g = S._npz("g5_mixedlen.npz")               # T = 8 observation block of the full-sensor fixture: 2 envs, navigation camera only
    B, T = 2, 8
    obs = {k[4:]: torch.from_numpy(v[:, :B]).to(DEV) for k, v in g.items() if k.startswith("obs:") and k[4:] not in ("manipulation_rgb_dinov2", "an_object_is_in_hand")}
    rs = np.random.RandomState(5)
    st = RolloutStorage(T, device=DEV, manip_uuid=None)
    st.initialize({k: v[0] for k, v in obs.items()}, num_samplers=B)
    assert st.observations["dino_tokens"].shape == (T + 1, B, 1, 84, 384) and "an_object_is_in_hand" not in st.observations
    pa, mk = g["prev_actions"][:, :B], g["masks"][:, :B]
    for t in range(T):
        nxt = {k: v[(t + 1) % T] for k, v in obs.items()}                            # step T wraps to the first block: the bootstrap observation is unused here
        st.add(nxt, None, torch.from_numpy(pa[(t + 1) % T]).to(DEV), torch.from_numpy(g["batch:old_action_log_probs"][t, :B]).to(DEV),
               torch.from_numpy(g["batch:values"][t, :B]).to(DEV), torch.from_numpy(rs.standard_normal((B, 1)).astype(np.float32)).to(DEV),
               torch.from_numpy(rs.binomial(5, 0.2, (B, 1)).astype(np.float32)).to(DEV), torch.from_numpy(g["batch:c_returns"][t, :B]).to(DEV),
               torch.from_numpy(mk[(t + 1) % T]).to(DEV))
    st.actions.copy_(torch.from_numpy(g["batch:actions"][:T, :B]).to(DEV))
    tok = st.observations["dino_tokens"][:T].float().cpu()
    robs = {k: v[:T].cpu() for k, v in st.observations.items() if k != "dino_tokens"}
    robs["rgb_dinov2"] = tok[:, :, 0].permute(0, 1, 3, 2).reshape(T, B, 384, 7, 12).contiguous()     # the storage's bf16 tokens, as the oracle's input
    ref = S.SubsetSafeActorCritic(GoalTokenizer(), max_batch=B).eval()
    ref.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
    nv, ncv = 0.3 * torch.ones(B, 1), -0.2 * torch.ones(B, 1)
    cfg = PPOLagConfig(update_repeats=1, cost_limit=2.0)
    eng = PPOLagEngine(model, cfg)
    info = eng.update(st, nv.to(DEV), ncv.to(DEV), episode_cost_sum=30.0, n_episodes=6.0)
    ret, adv = gae_scan(st.rewards.cpu(), st.value_preds[:T].cpu(), st.masks.cpu(), nv)
    cret, cadv = gae_scan(st.costs.cpu(), st.c_value_preds[:T].cpu(), st.masks.cpu(), ncv)
    lam = RefLagrange(2.0, 0.001, 0.035).update(5.0)
    cb = {"actions": st.actions.cpu(), "old_action_log_probs": st.action_log_probs.cpu(), "adv_targ": adv, "c_adv_targ": cadv, "returns": ret,
          "values": st.value_preds[:T].cpu(), "c_returns": cret}
    out, _ = ref(robs, None, st.prev_actions[:T].cpu(), st.masks[:T].cpu())
    total, ri = ref_loss.safe_ppo_log_grad(out["logits"], out["values"], cb, lam)
    c_loss = ref_loss.safe_ppo_value(out["c_values"], cret)
    assert abs(info["lagrangian_multiplier"] - lam) < 1e-6 and info["env_steps"] == T * B and eng.opt_step == 1
    got, want = [info["value"], info["action"], info["entropy"], info["c_value"]], [ri["value"], ri["action"], ri["entropy"], c_loss.item()]
    print("[nav-only engine update] losses gpu", got, "restatement", want)
    np.testing.assert_allclose(got, want, rtol=3e-2, atol=3e-2)                      # test_engine_gpu.py::test_chunked_accumulation_is_exact_and_matches_oracle
    assert torch.isfinite(model.arena.flat_p).all() and float((model.arena.flat_p - p_alike).abs().max()) > 0


def test_il_to_rl_handoff_between_models_of_the_same_cameras():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from safevla_amd.checkpoint import init_towers_from_il
    from safevla_amd.il import EarlyFusionCnnTransformer
    from safevla_amd.model import SafeDinoLLAMATxNavActorCriticSeparate

    nav16 = SafeDinoLLAMATxNavActorCriticSeparate(device=DEV, full_sensor=False)
    assert nav16.ncam == 1 and not nav16.has_hand and nav16.uuids["manip"] is None
    il = EarlyFusionCnnTransformer.build_model("small_3", [NAV, "last_actions"], device=DEV)
    ck = {"state_dict": {"model." + k: v.detach().cpu() + 0.125 for k, v in il.state_dict().items()}}
    for (loaded, missing, extra), tower in zip(init_towers_from_il(nav16, ck), nav16.towers):
        assert not extra and all(k.startswith("critic.") for k in missing), (missing[:4], extra[:4])
        assert torch.equal(tower.actor.linear.weight.detach().cpu(), ck["state_dict"]["model.actor.weight"])
        assert torch.equal(tower.visual_encoder.visual_sensor_token_raw_navigation_camera.detach().cpu(), ck["state_dict"]["model.visual_encoder.visual_sensor_token_raw_navigation_camera"])
    # a checkpoint of the four-sensor set: the tensors the towers do not have are reported as unused, everything else loads
    il4 = EarlyFusionCnnTransformer.build_model("small_3", device=DEV)
    ck4 = {"state_dict": {"model." + k: v.detach().cpu() for k, v in il4.state_dict().items()}}
    for loaded, missing, extra in init_towers_from_il(nav16, ck4):
        assert sorted(extra) == ["object_in_hand_embed.weight", "visual_encoder.visual_sensor_token_raw_manipulation_camera"]


# ------------------------------------------------------------------------------------------------ around the model
def test_navigation_only_rollout_collection_fast_path_equals_three_stream_replay():
    """``synth_env`` emits only the configured observations; ``collect_rollout`` steps a navigation-only model through the staged, tower-grouped step
    (``_acting_fast``: svla_acting_stage with a NULL in-hand pair) and through the three-stream replay of the general path: same rollout, bit for bit."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from safevla_amd.model import SafeDinoLLAMATxNavActorCriticSeparate
    from safevla_amd.storage import RolloutStorage
    from safevla_amd.synth_env import SynthSpec, SynthVectorEnv, collect_rollout, fill_synthetic_rollout

    torch.manual_seed(5)
    m = SafeDinoLLAMATxNavActorCriticSeparate(device=DEV, full_sensor=False).eval()
    B, T = 4, 6
    res = {}
    for grouped in (True, False):
        m.grouped_towers = grouped
        for t in m.towers:
            t.time_step_counter, t._kv = 0, None
        env = SynthVectorEnv(B, L=7, task="ObjectNav", seed=3, max_steps=500, device=DEV, full_sensor=False)
        obs0 = env.reset()
        assert set(obs0) == {"goal_token_ids", "time_step", "traj_index", "dino_tokens"} and obs0["dino_tokens"].shape == (B, 1, 84, 384)
        st = RolloutStorage(T, device=DEV, manip_uuid=None)
        torch.manual_seed(9)
        nxt = collect_rollout(m, env, st, T, obs0=obs0)
        assert st.observations["dino_tokens"].shape == (T + 1, B, 1, 84, 384)
        res[grouped] = (st.actions.clone(), st.action_log_probs.clone(), st.value_preds.clone(), st.c_value_preds.clone(), nxt["next_value"].clone())
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b), float((a.float() - b.float()).abs().max())
    assert torch.isfinite(res[True][1]).all() and float(res[True][2].abs().sum()) > 0
    # the full-sequence generator follows the model's sensor set too
    st, nxt, _ = fill_synthetic_rollout(m, SynthSpec(T=4, B=2, L=7, task="ObjectNav", seed=2), device=DEV)
    assert st.observations["dino_tokens"].shape == (5, 2, 1, 84, 384) and "an_object_is_in_hand" not in st.observations


def test_navigation_only_inference_agent_and_single_camera_preprocessing():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from safevla_amd.agent import ALL_STRETCH_ACTIONS, NAV_ACTIONS, InferenceAgentVIDA
    from safevla_amd.model import SafeDinoLLAMATxNavActorCriticSeparate

    torch.manual_seed(6)
    m = SafeDinoLLAMATxNavActorCriticSeparate(device=DEV, full_sensor=False)
    m.mask_non_nav_actions()
    agent = InferenceAgentVIDA.build_agent(m, device=DEV)
    assert agent.manip_pre is None
    rs = np.random.RandomState(1)
    for step in range(3):
        # a manipulation frame and an in-hand flag in the evaluator's dict are not read by a policy without these sensors
        frame = {"raw_navigation_camera": rs.randint(0, 256, (224, 384, 3), dtype=np.uint8), "an_object_is_in_hand": [1]}
        a, p = agent.get_action(frame, "find a mug")
        assert a in NAV_ACTIONS and p.shape == (20,) and abs(float(p.sum()) - 1.0) < 1e-4
        assert (p[[i for i, n in enumerate(ALL_STRETCH_ACTIONS) if n not in NAV_ACTIONS]] == 0).all()
    assert agent.rollout_storage.observations["dino_tokens"].shape[2:] == (1, 84, 384) and "an_object_is_in_hand" not in agent.rollout_storage.observations
    # one pass over "all" cameras of a single-camera storage == the per-camera call
    fr = torch.from_numpy(rs.randint(0, 256, (3, 224, 384, 3), dtype=np.uint8)).to(DEV)
    a1 = torch.zeros(3, 1, 84, 384, device=DEV, dtype=torch.bfloat16)
    b1 = torch.zeros_like(a1)
    agent.nav_pre.process_tokens(fr, a1, cam=0, ncam=1)
    agent.nav_pre.process_tokens_all_cameras(fr, b1)
    assert torch.equal(a1, b1) and float(a1.float().abs().sum()) > 0

