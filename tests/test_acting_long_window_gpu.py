"""Acting through episodes longer than 512 steps: the KV-cached policy step over a cache window of up to 1024 slots (csrc/attn_decode.hip), on the plain,
the recorded and the tower-grouped acting paths of the three-tower model, in the fp32 verification mode, and in the imitation-learning model's online agent.

The reference evaluates online on episodes of 600 steps (1000 for RoomVisit / ObjectNavMulti) and builds its policies and llama caches for 1000; every step
attends to all steps of its episode so far.  Before the long window existed the plain path stopped at step 512 with an ``SvlaError``, the recorded path (which
attends over all ``max_steps`` slots behind a mask) at its first step, and the IL agent restarted its window at step 512 with a warning."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, L, RESTART = 530, 12, 397          # acting steps; goal tokens; the step at which env 1 begins a new episode (its window then crosses slot 512 with a late start)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _episodes(envs):
    """N steps of synthetic observations for the given envs (0: one episode from step 0; 1: a new episode at step RESTART), the storage-native layout of one
    acting step per index: dino tokens [N, B, 2, 84, 384] bf16 drawn from a pool of 41 frames, goal ids, time_step, traj_index, hand, prev_actions, masks."""
    g = torch.Generator().manual_seed(5)
    pool = torch.randn(41, 2, 84, 384, generator=g).to(torch.bfloat16)
    goals = torch.randint(3, 32000, (2, 2, L), generator=g)
    goals[..., -1] = 1
    prev = torch.randint(0, 20, (N, 2), generator=g)
    hand = torch.randint(0, 2, (N, 2, 1), generator=g)
    t = torch.arange(N)
    start = torch.tensor([0, RESTART])
    ep = (t[:, None] >= start[None, :]).long() * (start[None, :] > 0).long()          # episode index of (step, env)
    ts = t[:, None] - ep * start[None, :]
    masks = (ts != 0).float()[..., None]
    obs = {"dino_tokens": pool[(7 * t[:, None] + 13 * torch.arange(2)[None, :]) % 41], "goal_token_ids": goals[torch.arange(2)[None, :], ep], "time_step": ts,
           "traj_index": ep + 10 * torch.arange(2)[None, :], "an_object_is_in_hand": hand}
    e = list(envs)
    return {k: v[:, e].contiguous().to(DEV) for k, v in obs.items()}, prev[:, e].contiguous().to(DEV), masks[:, e].contiguous().to(DEV)


def _act(m, obs, prev, masks, mode, steps=range(N)):
    """fresh caches, then one acting step per index of ``steps``; per step (log-probs, values, cost values)"""
    for t in m.towers:
        t.time_step_counter, t._kv = 0, None
    if mode == "plain":                      # S_att = t + 1, kvalid built per step
        m.enable_acting_graphs(False)
    elif m.precision == "bf16":              # recorded launch plans (S_att = max_steps behind kvalid_static): tower-grouped replay, or one stream per tower
        m.grouped_towers = mode == "grouped"
        m.enable_acting_plans(True)
    out = []
    try:
        with torch.no_grad():
            for t in steps:
                o, _ = m({k: v[t:t + 1] for k, v in obs.items()}, None, prev[t:t + 1], masks[t:t + 1])
                out.append(torch.cat([torch.log_softmax(o.distributions.logits.float(), -1).reshape(-1, 20), o.values.float().reshape(-1, 1),
                                      o.c_values.float().reshape(-1, 1)], 1))
        torch.cuda.synchronize()
    finally:
        if m.precision == "bf16":
            m.grouped_towers = True
            m.enable_acting_plans(True)
    assert all(t.time_step_counter == len(out) for t in m.towers)
    return torch.stack(out).cpu()            # [steps, B, 22]


@pytest.fixture(scope="module")
def model():
    _need_gpu()
    from oracle.detfill import fill_state_dict
    from safevla_amd.model import SafeDinoLLAMATxNavActorCriticSeparate

    m = SafeDinoLLAMATxNavActorCriticSeparate(device=DEV, max_steps=1000)
    fill_state_dict(m, seed=3)
    m.sync_weights()
    return m.eval()


@pytest.fixture(scope="module")
def runs(model):
    """the 530 steps at 2 envs on the three acting paths (computed once)"""
    obs, prev, masks = _episodes((0, 1))
    return {mode: _act(model, obs, prev, masks, mode) for mode in ("grouped", "streams", "plain")}


def _rel(a, b):
    """largest error relative to the largest reference value, log-probs / values / cost values apart (the metric of tests/test_model_gpu.py)"""
    return [float((a[..., s] - b[..., s]).abs().max() / (b[..., s].abs().max() + 1e-12)) for s in (slice(0, 20), slice(20, 21), slice(21, 22))]


def test_recorded_and_plain_paths_agree_beyond_step_512(runs):
    """gate: test_model_gpu.py::test_fused_rmsnorm_step_close_to_unfused / test_acting_graph_replay_equals_eager_acting (2e-2 of the largest value)"""
    g, p = runs["grouped"], runs["plain"]
    assert torch.isfinite(g).all() and torch.isfinite(p).all()
    e_all, e_late = _rel(g, p), _rel(g[512:], p[512:])
    print(f"recorded / grouped vs plain acting steps, rel-to-max [log p, v, c]: all steps {e_all}, steps >= 512 {e_late}")
    assert max(e_late) < 2e-2 and max(e_all) < 2e-2
    assert float((g[512:] - g[511:-1]).abs().max()) > 1e-3            # (the policy's outputs do move from step to step)


def test_grouped_replay_equals_three_stream_replay_bit_for_bit(runs):
    assert torch.equal(runs["grouped"], runs["streams"])


def test_late_start_episode_equals_the_same_episode_from_slot_zero(model, runs):
    """Env 1's second episode sits in cache slots 397 ... 529; fed alone to fresh caches it sits in slots 0 ... 132: same keys, other slots, other row count.
    Gate: the bf16 acting gate of tests/test_model_gpu.py (3e-2 of the largest value)."""
    obs, prev, masks = _episodes((1,))
    fresh = _act(model, obs, prev, masks, "grouped", steps=range(RESTART, N))
    e = _rel(runs["grouped"][RESTART:, 1:2], fresh)
    print(f"episode at slots {RESTART}..{N - 1} vs the same episode at slots 0..{N - 1 - RESTART}, rel-to-max [log p, v, c]: {e}")
    assert max(e) < 3e-2


def test_bf16_and_fp32_modes_agree_over_530_steps(model):
    """gate: the project's bf16 product path vs fp32 (2e-2 of the largest logit / value)"""
    from safevla_amd.model import SafeDinoLLAMATxNavActorCriticSeparate

    obs, prev, masks = _episodes((0,))
    got = _act(model, obs, prev, masks, "grouped")
    m32 = SafeDinoLLAMATxNavActorCriticSeparate(device=DEV, max_steps=1000, precision="fp32").eval()
    m32.load_state_dict(model.state_dict())
    want = _act(m32, obs, prev, masks, "plain")
    del m32
    e_all, e_late = _rel(got, want), _rel(got[512:], want[512:])
    print(f"bf16 vs fp32 mode, rel-to-max [log p, v, c]: all steps {e_all}, steps >= 512 {e_late}")
    assert torch.isfinite(want).all() and max(e_all) < 2e-2


def test_a_window_above_1024_steps_is_refused_at_construction():
    _need_gpu()
    from safevla_amd.model import SafeDinoLLAMATxNavActorCriticSeparate

    with pytest.raises(ValueError, match="1024"):
        SafeDinoLLAMATxNavActorCriticSeparate(device=DEV, max_steps=1025)


def test_il_agent_attends_to_the_whole_episode_up_to_1000_steps():
    _need_gpu()
    from oracle.detfill import fill_state_dict
    from safevla_amd.il import EarlyFusionCnnTransformer, EarlyFusionCnnTransformerAgent

    agent = EarlyFusionCnnTransformer.build_agent("small_3", device=DEV, sampling="greedy")
    assert agent.max_seq_len == 1000
    m = agent.model
    fill_state_dict(m, seed=17, share_t5=False)
    m.sync_weights()
    m.eval()
    rs = np.random.RandomState(8)
    pool = rs.standard_normal((2, 23, 384, 7, 12)).astype(np.float32)
    goal = dict(input_ids=np.array([[917, 4033, 88, 21, 1]]), attention_mask=np.ones((1, 5), np.int64))
    step = lambda a, t: a.get_action({"raw_navigation_camera": pool[0, t % 23], "raw_manipulation_camera": pool[1, (3 * t) % 23], "an_object_is_in_hand": [t % 2]}, goal)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for t in range(520):
            _, p = step(agent, t)
            if t % 40 == 0 or t >= 510:
                assert p.shape == (20,) and bool(torch.isfinite(p).all()) and abs(float(p.sum()) - 1.0) < 1e-4, t
    assert agent.curr_t == 520 and m.time_step_counter == 520
    # a window shorter than the episode: the restart and its warning are what they were
    small = EarlyFusionCnnTransformerAgent(m, DEV, "greedy", max_seq_len=8)
    assert small.max_seq_len == 8
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for t in range(8):
            step(small, t)
    assert m.time_step_counter == 8
    with pytest.warns(UserWarning, match="window restarts"):
        step(small, 8)
    assert small.curr_t == 9 and m.time_step_counter == 1
    with warnings.catch_warnings():
        warnings.simplefilter("error")          # one warning per episode
        for t in range(9, 17):
            step(small, t)
    assert m.time_step_counter == 1
