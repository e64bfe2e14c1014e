"""``EarlyFusionCnnTransformerVectorAgent``: several online episodes of the imitation-learning model on per-row KV rings behind one set of weights
(safevla_amd/il.py; csrc/attn_decode.hip; the fusion encoder's key-padding mask).

Reference of every check: ``forward(batch)`` of the same model on ONE episode alone (B = 1, its goal unpadded, ``last_actions`` = the agent's own actions shifted,
start token first) -- the comparison of tests/test_il_gpu.py::test_il_agent_steps_equal_full_sequence_forward, and its gate: 2e-2 * max(ref.max(), 1e-3) on the
action probabilities of every step (tests/helpers/vector_agents.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers.vector_agents import Episode as _Episode, gate as _gate, staggered_episodes      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
VERSIONS = ["small_3", "siglip_base_6_3"]
_MODELS = {}


def _model(version):
    """one model per preset for the whole module: fill_state_dict(seed=17), eval mode"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    if version not in _MODELS:
        from oracle.detfill import fill_state_dict
        from safevla_amd.il import EarlyFusionCnnTransformer

        m = EarlyFusionCnnTransformer.build_model(version, device=DEV)
        fill_state_dict(m, seed=17, share_t5=False)
        m.sync_weights()
        _MODELS[version] = m.eval()
    return _MODELS[version]


def _vector_agent(m, n, **kw):
    from safevla_amd.il import EarlyFusionCnnTransformerVectorAgent

    return EarlyFusionCnnTransformerVectorAgent(m, n, DEV, **kw)


def _goal(m, rs, n_tokens):
    """a goal of ``n_tokens`` tokens: t5 ids ending in the end-of-sequence token 1; SigLIP: the fixed context of 64 padded with 1"""
    if m.text_encoder_name == "t5-small":
        ids = np.concatenate([rs.randint(3, 32000, n_tokens - 1), [1]])[None]
        return dict(input_ids=ids, attention_mask=np.ones_like(ids))
    ids = np.ones((1, 64), np.int64)
    ids[0, :n_tokens] = rs.randint(3, 32000, n_tokens)
    return ids


def _frame(m, rs):
    return {"raw_navigation_camera": rs.standard_normal((m.dino_dim, 7, 12)).astype(np.float32),
            "raw_manipulation_camera": rs.standard_normal((m.dino_dim, 7, 12)).astype(np.float32), "an_object_is_in_hand": [int(rs.randint(0, 2))]}


def _forward_probs(m, frames, goal, time_ids, last_actions):
    """action probabilities [T, 20] of forward(batch) on one episode alone"""
    goals = {k: torch.as_tensor(v).to(DEV) for k, v in goal.items()} if isinstance(goal, dict) else torch.as_tensor(goal).to(DEV)
    stack = lambda k: torch.from_numpy(np.stack([f[k] for f in frames]))[None].to(DEV)
    batch = {"raw_navigation_camera": stack("raw_navigation_camera"), "raw_manipulation_camera": stack("raw_manipulation_camera"),
             "time_ids": torch.tensor([list(time_ids)], device=DEV), "an_object_is_in_hand": torch.tensor([[f["an_object_is_in_hand"][0] for f in frames]], device=DEV),
             "last_actions": torch.tensor([list(last_actions)], device=DEV), "goals": goals}
    with torch.no_grad():
        return torch.softmax(m(batch)["actions_logits"][0].float(), -1).cpu().numpy()


@pytest.mark.parametrize("version", VERSIONS)
def test_staggered_episodes_equal_their_own_forward(version):
    """Three slots with goals of 3, 5 and 7 tokens that start at calls 0, 2 and 4; slot 1 sits out calls 5 and 6; slot 0 is reset after 5 steps with a goal of
    another length; 12 calls.  Every finished episode equals the B = 1 forward of that episode alone: padded goal tokens are hidden, no slot's cache is touched by
    another slot's step, a stalled slot does not age."""
    m = _model(version)
    rs = np.random.RandomState(8)
    lengths = {0: 3, 1: 5, 2: 7, "reset": 4}
    done = staggered_episodes(_vector_agent(m, 3), lambda s: _goal(m, rs, lengths[s]), lambda: _frame(m, rs))
    for i, e in enumerate(done):
        ref = _forward_probs(m, e.frames, e.goal, range(len(e.acts)), [20] + e.acts[:-1])
        _gate(np.stack(e.probs), ref, f"{version} episode {i} ({len(e.acts)} steps)")


@pytest.mark.parametrize("version", VERSIONS)
def test_ring_slides_over_the_last_window_steps(version):
    """max_seq_len = 8, 13 steps in slot 0: from step 8 on the episode attends to its last 8 steps, and the step's probabilities are those of the last position of
    forward(batch) on steps t - 7 ... t (their time_ids, the agent's actions shifted).  A second slot starts at step 3 and steps in between -- from step 9 on in
    one batch with the slot that has outlived its window: it leaves slot 0 alone and equals its own B = 1 forward."""
    m = _model(version)
    rs = np.random.RandomState(9)
    agent = _vector_agent(m, 2, max_seq_len=8)
    ep, other = _Episode(_goal(m, rs, 5)), _Episode(_goal(m, rs, 3))
    agent.reset(0, ep.goal)
    for t in range(13):
        if t == 3:
            agent.reset(1, other.goal)
        frames = {0: _frame(m, rs)}
        if t in (3, 4, 6, 9, 10, 12):
            frames[1] = _frame(m, rs)
        out = agent.get_actions(frames)
        ep.record(agent, frames[0], out[0])
        if 1 in frames:
            other.record(agent, frames[1], out[1])
    assert agent.age(0) == 13 and agent.age(1) == 6
    last = [20] + ep.acts[:-1]
    figures = []
    for t in range(8, 13):
        ref = _forward_probs(m, ep.frames[t - 7:t + 1], ep.goal, range(t - 7, t + 1), last[t - 7:t + 1])[-1]
        figures.append((float(np.abs(ep.probs[t] - ref).max()), 2e-2 * max(float(ref.max()), 1e-3)))
        print(f"{version} step {t} vs forward on steps {t - 7} ... {t}: max |dp| {figures[-1][0]:.3e}, gate {figures[-1][1]:.3e}")
    assert all(err < tol for err, tol in figures), figures
    _gate(np.stack(ep.probs[:8]), _forward_probs(m, ep.frames[:8], ep.goal, range(8), last[:8]), f"{version} steps 0 ... 7")
    _gate(np.stack(other.probs), _forward_probs(m, other.frames, other.goal, range(6), [20] + other.acts[:-1]), f"{version} second slot")


def test_api_sampling_slots_and_the_single_agent_afterwards():
    from safevla_amd.il import EarlyFusionCnnTransformer, EarlyFusionCnnTransformerAgent

    m = _model("small_3")
    rs = np.random.RandomState(10)
    with pytest.raises(NotImplementedError, match="64-wide decoder heads"):
        EarlyFusionCnnTransformer.build_vector_agent("base_6", device=DEV, num_episodes=2)
    for n in (0, 1025):
        with pytest.raises(ValueError):
            _vector_agent(m, n)
    gen = torch.Generator(device=DEV)
    agent = _vector_agent(m, 4, sampling="sample", generator=gen)
    goals = {0: _goal(m, rs, 4), 2: _goal(m, rs, 6)}
    frames = [{s: _frame(m, rs) for s in goals} for _ in range(4)]
    m.time_step_counter = counter = 3
    draws = []
    for _ in range(2):                                                      # the same seed, goals and frames after a reset: the same draws
        gen.manual_seed(1234)
        for s, g in goals.items():
            agent.reset(s, g)
        run = []
        for f in frames:
            out = agent.get_actions(f)
            for s in goals:
                assert out[s][0] in agent.get_action_list() and out[s][1].shape == (20,) and abs(float(out[s][1].sum()) - 1.0) < 1e-4
            run.append([out[s][0] for s in goals])
        draws.append(run)
    assert draws[0] == draws[1]
    assert m.time_step_counter == counter                                   # vector steps neither read nor advance the tower's own counter
    assert agent.age(0) == 4 and agent.age(2) == 4
    for bad in (1, 3, 4, -1, "0"):                                          # never started / out of range / not a slot
        with pytest.raises(KeyError):
            agent.get_actions({bad: frames[0][0]})
    with pytest.raises(KeyError):
        agent.age(1)
    with pytest.raises(KeyError):
        agent.reset(4, goals[0])
    with pytest.raises(ValueError):
        agent.get_actions({})
    # a single agent built afterwards on the same model: three steps against forward(batch)
    single = EarlyFusionCnnTransformerAgent(m, DEV)
    ep = _Episode(_goal(m, rs, 5))
    for _ in range(3):
        f = _frame(m, rs)
        ep.record(single, f, single.get_action(f, ep.goal))
    _gate(np.stack(ep.probs), _forward_probs(m, ep.frames, ep.goal, range(3), [20] + ep.acts[:-1]), "single agent after vector steps")


def test_fusion_key_mask_is_forward_only():
    m = _model("small_3")
    rs = np.random.RandomState(11)
    goal = _goal(m, rs, 5)
    f = _frame(m, rs)
    batch = {"raw_navigation_camera": torch.from_numpy(f["raw_navigation_camera"])[None, None].to(DEV),
             "raw_manipulation_camera": torch.from_numpy(f["raw_manipulation_camera"])[None, None].to(DEV), "time_ids": torch.zeros(1, 1, dtype=torch.int64, device=DEV),
             "an_object_is_in_hand": torch.zeros(1, 1, dtype=torch.int64, device=DEV), "last_actions": torch.full((1, 1), 20, device=DEV),
             "goals": {k: torch.as_tensor(v).to(DEV) for k, v in goal.items()}}
    prep = m.prepare(batch)
    prep.fusion_kvalid = torch.ones(prep.R, prep.S, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="fusion_kvalid"):
        m.run_forward(prep, need_grad=True)
    with torch.no_grad():
        masked, _, _ = m.run_forward(prep, need_grad=False)                 # an all-ones mask hides nothing
        prep.fusion_kvalid = None
        plain, _, _ = m.run_forward(prep, need_grad=False)
    assert (masked - plain).abs().max() <= 2e-2 * plain.abs().max()
