"""``agent.VectorInferenceAgentVIDA``: several online evaluation episodes of the RL policy on per-row KV rings behind one set of weights, actor tower only
(safevla_amd/agent.py; csrc/attn_decode.hip; csrc/sample.hip; the fusion encoder's key-padding mask).

Reference of every check: the same model's sequence forward on ONE episode alone -- ``forward(observations, memory, prev_actions, masks)`` at T = len, B = 1, under
no_grad in eval mode, a constant ``traj_index``, the goal unpadded, ``prev_actions`` = the agent's own sampled actions shifted by one, ``masks[0] = 0`` -- and the gate
of tests/test_il_vector_agent_gpu.py: 2e-2 * max(ref.max(), 1e-3) on the action probabilities of every step.  (The forwards on steps 8 ... t of the window test do
not start an episode: their first step has a previous action and ``masks`` = 1, as the agent and the reference's step counter have it at a cache restart.)"""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers.vector_agents import Episode as _Episode, gate as _gate, staggered_episodes      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAV_IDS = [0, 1, 2, 3, 4, 6, 7]          # m, r, l, b, end, ls, rs of agent.ALL_STRETCH_ACTIONS
_MODELS = {}


def _model(kind):
    """one model per kind for the whole module -- "full": four sensors; "nav": full_sensor=False; "w8": four sensors, max_steps = 8.  fill_state_dict(seed=7), eval"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    if kind not in _MODELS:
        from oracle.detfill import fill_state_dict
        from safevla_amd.model import SafeDinoLLAMATxNavActorCriticSeparate

        m = SafeDinoLLAMATxNavActorCriticSeparate(device=DEV, full_sensor=kind != "nav", **(dict(max_steps=8) if kind == "w8" else {}))
        fill_state_dict(m, seed=7)
        m.sync_weights()
        _MODELS[kind] = m.eval()
    return _MODELS[kind]


def _vector_agent(m, n, **kw):
    from safevla_amd.agent import InferenceAgentVIDA

    return InferenceAgentVIDA.build_vector_agent(m, num_episodes=n, device=DEV, **kw)


def _goal(rs, n_tokens):
    """a goal of ``n_tokens`` t5 ids ending in the end-of-sequence token 1"""
    ids = np.concatenate([rs.randint(3, 32000, n_tokens - 1), [1]])[None]
    return dict(input_ids=ids, attention_mask=np.ones_like(ids))


def _frame(rs):
    """already-encoded features under the model's uuids (no ViT).  Always the full set: a navigation-only model must not read the other two"""
    return {"rgb_dinov2": rs.standard_normal((384, 7, 12)).astype(np.float32), "manipulation_rgb_dinov2": rs.standard_normal((384, 7, 12)).astype(np.float32),
            "an_object_is_in_hand": [int(rs.randint(0, 2))]}


def _forward_probs(m, frames, goal, time_steps, prev_actions, first_mask=0.0):
    """action probabilities [T, 20] of the model's sequence forward on one episode alone"""
    u, T = m.uuids, len(frames)
    ids = m.tokenizer.encode(goal) if isinstance(goal, str) else np.asarray(goal["input_ids"]).reshape(-1).tolist()
    col = lambda v: torch.as_tensor(np.asarray(list(v)), dtype=torch.int64).reshape(T, 1).to(DEV)
    stack = lambda k: torch.from_numpy(np.stack([f[k] for f in frames]))[:, None].to(DEV)
    obs = {u["nav"]: stack("rgb_dinov2"), "goal_token_ids": torch.tensor(ids, dtype=torch.int64, device=DEV).reshape(1, 1, -1).repeat(T, 1, 1), u["time"]: col(time_steps),
           u["traj"]: torch.full((T, 1), 3, dtype=torch.int64, device=DEV)}
    if u["manip"] is not None:
        obs[u["manip"]] = stack("manipulation_rgb_dinov2")
    if u["hand"] is not None:
        obs[u["hand"]] = col(f["an_object_is_in_hand"][0] for f in frames)
    mk = torch.ones(T, 1, 1, device=DEV)
    mk[0] = first_mask
    if T == 1:                                                              # a one-step forward is a step against the towers' KV caches: at counter 0 it sees itself alone
        for t in m.towers:
            t.time_step_counter = 0
    with torch.no_grad():
        out, _ = m(obs, None, col(prev_actions), mk)
    return out.distributions.probs[:, 0].float().cpu().numpy()


def _check(e, m, name):
    n = len(e.acts)
    _gate(np.stack(e.probs), _forward_probs(m, e.frames, e.goal, range(n), [0] + e.acts[:-1]), f"{name} ({n} steps)")


@pytest.mark.parametrize("kind", ["full", "nav"])
def test_staggered_episodes_equal_their_own_forward(kind):
    """Three slots with goals of 3, 5 (a string) and 7 tokens that start at calls 0, 2 and 4; slot 1 sits out calls 5 and 6; slot 0 is reset after 5 steps with a goal of
    another length; 12 calls.  Every finished episode equals the B = 1 forward of that episode alone: padded goal tokens are hidden, no slot's cache is touched by
    another slot's step, a stalled slot does not age.  Once on the full sensor set, once with full_sensor=False (one camera, no in-hand sensor)."""
    m = _model(kind)
    rs = np.random.RandomState(8)
    goals = {0: _goal(rs, 3), 1: "find a red mug", 2: _goal(rs, 7)}
    assert len(m.tokenizer.encode(goals[1])) == 5
    done = staggered_episodes(_vector_agent(m, 3, seed=21), lambda s: goals[s] if s in goals else _goal(rs, 4), lambda: _frame(rs))
    for i, e in enumerate(done):
        _check(e, m, f"{kind} episode {i}")


def test_only_the_actor_tower_is_launched():
    """A trace of every C-ABI call of two vector steps: no argument points into the critics' ranges of the weight arena (fp32 masters, bf16 mirror) -- while arguments
    do point into the actor's, so the trace sees weights --; the critics' KV caches keep a sentinel, their step counters stand."""
    from safevla_amd import ops

    m = _model("full")
    rs = np.random.RandomState(12)
    agent = _vector_agent(m, 2)
    critics = m.towers[1:]
    for t in critics:
        t._ensure_caches(2)
        for c in t._kv:
            c.fill_(7.0)
    counters = [t.time_step_counter for t in m.towers]
    for s in range(2):
        agent.reset(s, _goal(rs, 3 + 2 * s))
    ar, lib = m.arena, ops.lib()
    spans = lambda k: [(f.data_ptr() + ar.tower_ranges[k][0] * f.element_size(), f.data_ptr() + ar.tower_ranges[k][1] * f.element_size()) for f in (ar.flat_p, ar.flat_bf16)]
    inside = lambda args, k: any(isinstance(a, int) and lo <= a < hi for a in args for lo, hi in spans(k))
    lib.recorder = []
    try:
        for _ in range(2):
            agent.get_actions({s: _frame(rs) for s in range(2)})
        trace = lib.recorder
    finally:
        lib.recorder = None
    torch.cuda.synchronize()
    assert len(trace) > 50 and sum(inside(args, 0) for _, args in trace) > 20       # the actor's weights are seen
    assert not any(inside(args, 1) or inside(args, 2) for _, args in trace)
    assert all(bool((c == 7.0).all()) for t in critics for c in t._kv)
    assert [t.time_step_counter for t in m.towers] == counters


def test_window_restarts_at_max_steps():
    """max_steps = 8, 11 steps in one slot.  Steps 0 ... 7 equal the forward on steps 0 ... 7; steps 8 ... 10 -- after the cache restart of the reference's step counter
    (allenact_dino_transformer.py:376-377) -- equal the last position of the forward on steps 8 ... t with their own time_step values (10 at t = 10, not 2), the
    previous actions and masks of those steps.  One warning."""
    m = _model("w8")
    rs = np.random.RandomState(9)
    agent = _vector_agent(m, 2, seed=5)
    ep = _Episode(_goal(rs, 5))
    agent.reset(1, ep.goal)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for t in range(11):
            f = _frame(rs)
            ep.record(agent, f, agent.get_actions({1: f})[1])
    assert agent.age(1) == 11
    assert len([w for w in caught if "KV-cache window" in str(w.message)]) == 1, [str(w.message) for w in caught]
    last = [0] + ep.acts[:-1]
    _gate(np.stack(ep.probs[:8]), _forward_probs(m, ep.frames[:8], ep.goal, range(8), last[:8]), "steps 0 ... 7")
    figures = []
    for t in range(8, 11):
        ref = _forward_probs(m, ep.frames[8:t + 1], ep.goal, range(8, t + 1), last[8:t + 1], first_mask=1.0)[-1]
        figures.append((float(np.abs(ep.probs[t] - ref).max()), 2e-2 * max(float(ref.max()), 1e-3)))
        print(f"step {t} vs forward on steps 8 ... {t}: max |dp| {figures[-1][0]:.3e}, gate {figures[-1][1]:.3e}")
    assert all(err < tol for err, tol in figures), figures


def test_sampled_actions_do_not_depend_on_the_other_slots():
    """The same episode, the same seed: alone in slot 2, and beside two live slots with goals of other lengths (so its goal is padded).  Identical sampled actions
    (the draw is a function of seed, slot and age; the agent is not greedy), probabilities within the gate."""
    m = _model("full")
    rs = np.random.RandomState(13)
    goal, frames = _goal(rs, 4), [_frame(rs) for _ in range(6)]
    others = {0: _goal(rs, 7), 1: _goal(rs, 3)}
    runs = []
    for crowd in (False, True):
        agent = _vector_agent(m, 3, seed=99)
        ep = _Episode(goal)
        agent.reset(2, goal)
        for s, g in others.items() if crowd else ():
            agent.reset(s, g)
            agent.get_actions({s: _frame(rs)})                              # other ages than slot 2's
        for f in frames:
            call = {2: f, **({s: _frame(rs) for s in others} if crowd else {})}
            ep.record(agent, f, agent.get_actions(call)[2])
        runs.append(ep)
    assert runs[0].acts == runs[1].acts, (runs[0].acts, runs[1].acts)
    _gate(np.stack(runs[1].probs), np.stack(runs[0].probs), "beside two slots vs alone")
    other_seed = _vector_agent(m, 3, seed=100)
    other_seed.reset(2, goal)
    acts = [other_seed.get_action_list().index(other_seed.get_actions({2: f})[2][0]) for f in frames]
    print("seed 99:", runs[0].acts, "seed 100:", acts)
    assert acts != runs[0].acts                                             # seed= takes the place of generator=: another seed, other draws


def test_masked_policy_never_returns_a_non_navigation_action():
    """``mask_non_nav_actions()``: 200 sampled steps (8 slots x 25 calls) return navigation actions only, and every other action has probability exactly 0"""
    m = _model("nav")
    bias = m.actor.linear.bias.detach().clone()
    rs = np.random.RandomState(14)
    try:
        masked = m.mask_non_nav_actions()
        assert masked == [i for i in range(20) if i not in NAV_IDS]
        agent = _vector_agent(m, 8, seed=1)
        for s in range(8):
            agent.reset(s, _goal(rs, 3 + s % 3))
        names, seen = agent.get_action_list(), []
        for _ in range(25):
            out = agent.get_actions({s: _frame(rs) for s in range(8)})
            probs = torch.stack([out[s][1] for s in range(8)])
            assert bool((probs[:, masked] == 0).all())
            seen += [names.index(out[s][0]) for s in range(8)]
        assert len(seen) == 200 and set(seen) <= set(NAV_IDS) and len(set(seen)) > 1, sorted(set(seen))
    finally:
        with torch.no_grad():
            m.actor.linear.bias.copy_(bias)
        m.sync_weights(frozen=False)


def test_api_errors_and_the_single_agent_afterwards():
    from safevla_amd.agent import InferenceAgentVIDA, VectorInferenceAgentVIDA
    from safevla_amd.model import SafeDinoLLAMATxNavActorCriticSeparate

    m = _model("full")
    rs = np.random.RandomState(10)
    for n in (0, 1025):
        with pytest.raises(ValueError):
            _vector_agent(m, n)
    with pytest.raises(NotImplementedError, match="bf16 product path only"):
        VectorInferenceAgentVIDA(SafeDinoLLAMATxNavActorCriticSeparate(device=DEV, max_steps=8, precision="fp32"), 2, DEV)
    agent = _vector_agent(m, 4, greedy_sampling=True)
    goals = {0: _goal(rs, 4), 2: _goal(rs, 6)}
    for s, g in goals.items():
        agent.reset(s, g)
    counter = m.time_step_counter
    for _ in range(2):
        out = agent.get_actions({s: _frame(rs) for s in goals})
        for s in goals:                                                     # greedy: the most probable action is returned
            assert out[s][0] == agent.get_action_list()[int(out[s][1].argmax())]
    assert m.time_step_counter == counter and agent.age(0) == 2 and agent.age(2) == 2
    for bad in (1, 3, 4, -1, "0"):                                          # never started / out of range / not a slot
        with pytest.raises(KeyError):
            agent.get_actions({bad: _frame(rs)})
    with pytest.raises(KeyError):
        agent.age(1)
    with pytest.raises(KeyError):
        agent.reset(4, goals[0])
    with pytest.raises(ValueError):
        agent.get_actions({})
    # a single agent built afterwards on the same model: three steps on raw frames against the sequence forward over the same features
    single = InferenceAgentVIDA.build_agent(m, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5))
    raw = [{"raw_navigation_camera": rs.randint(0, 256, (224, 384, 3), dtype=np.uint8), "raw_manipulation_camera": rs.randint(0, 256, (224, 384, 3), dtype=np.uint8),
            "an_object_is_in_hand": np.array([int(i >= 1)])} for i in range(3)]
    acts, probs = [], []
    for f in raw:
        _, p = single.get_action(f, "find a red mug")
        acts.append(int(single.last_action_flat[0])); probs.append(p.float().cpu().numpy())
    feats = [{"rgb_dinov2": single.nav_pre.process({"rgb_raw": torch.from_numpy(f["raw_navigation_camera"])[None]})[0].cpu().numpy(),
              "manipulation_rgb_dinov2": single.manip_pre.process({"manipulation_rgb_raw": torch.from_numpy(f["raw_manipulation_camera"])[None]})[0].cpu().numpy(),
              "an_object_is_in_hand": f["an_object_is_in_hand"]} for f in raw]
    _gate(np.stack(probs), _forward_probs(m, feats, "find a red mug", range(3), [0] + acts[:-1]), "single agent after vector steps")
