"""il.Preprocessor: the reference's ``Preprocessor.process`` (architecture/models/transformer_models/preprocessors.py:76-310) for the sensors a model is built for --
a list of samples of unequal length -> one padded batch with ``lengths`` and ``padding_mask``.  Host code: runs with device="cpu".  Every padding value below is
the reference's (:105,124,143,200,212), restated; frames stay uint8 (the repository's convention: normalisation lives in the trunk's front)."""
import numpy as np
import pytest
import torch

NAV, MANIP = "raw_navigation_camera", "raw_manipulation_camera"
LENS = (5, 2, 1)
GOALS = ("find a mug", "go to the kitchen and look around", "apple")


def _actions():
    from safevla_amd.agent import ALL_STRETCH_ACTIONS
    return list(ALL_STRETCH_ACTIONS)


def _sample(rs, t, goal, extra=None, numpy_frames=False):
    A = _actions()
    acts = [A[i] for i in rs.randint(0, len(A), t)]
    frames = lambda: rs.randint(0, 256, (t, 4, 6, 3)).astype(np.uint8)
    obs = {NAV: frames() if numpy_frames else torch.from_numpy(frames()), MANIP: torch.from_numpy(frames()), "actions": acts, "last_actions": [""] + acts[:-1], "goal": goal,
           "time_ids": list(range(t)), "an_object_is_in_hand": rs.randint(0, 2, t), "initial_agent_location": [1.0, 0.9, 2.0, 0.0, 90.0, 0.0], "templated_task_type": "x"}
    obs.update(extra or {})
    return {"observations": obs}


@pytest.fixture(scope="module")
def samples():
    rs = np.random.RandomState(3)
    return [_sample(rs, t, g, numpy_frames=i == 1) for i, (t, g) in enumerate(zip(LENS, GOALS))]


def test_every_key_dtype_shape_and_padding_value(samples):
    from safevla_amd.il import PAD_TOKEN, START_TOKEN, Preprocessor
    from safevla_amd.text import GoalTokenizer

    A = _actions()
    pp = Preprocessor(device="cpu")
    out = pp.process(samples)
    B, T = len(LENS), max(LENS)
    assert set(out) == {NAV, MANIP, "actions", "last_actions", "goals", "time_ids", "an_object_is_in_hand", "lengths", "padding_mask"}      # the ignored keys are gone
    assert out["lengths"].dtype == torch.int32 and out["lengths"].tolist() == list(LENS)
    assert out["padding_mask"].dtype == torch.bool and out["padding_mask"].shape == (B, T)
    assert torch.equal(out["padding_mask"], torch.arange(T)[None, :] >= torch.tensor(LENS)[:, None])
    pad = out["padding_mask"]
    for cam in (NAV, MANIP):
        assert out[cam].dtype == torch.uint8 and out[cam].shape == (B, T, 4, 6, 3)
        assert (out[cam][pad] == 0).all()
        for b, s in enumerate(samples):
            assert torch.equal(out[cam][b, :LENS[b]], torch.as_tensor(s["observations"][cam]))
    for key, value in (("actions", -1), ("last_actions", PAD_TOKEN), ("an_object_is_in_hand", 2), ("time_ids", -1)):
        assert out[key].dtype == torch.int64 and out[key].shape == (B, T), key
        assert (out[key][pad] == value).all(), key
    assert PAD_TOKEN == 21 and START_TOKEN == 20 and pp.num_actions == 21
    for b, s in enumerate(samples):
        o, n = s["observations"], LENS[b]
        assert out["actions"][b, :n].tolist() == [A.index(a) for a in o["actions"]]
        assert out["last_actions"][b, :n].tolist() == [START_TOKEN] + [A.index(a) for a in o["actions"][:-1]]          # "" -> 20
        assert out["an_object_is_in_hand"][b, :n].tolist() == list(o["an_object_is_in_hand"])
        assert out["time_ids"][b, :n].tolist() == list(range(n))
    want = GoalTokenizer()(list(GOALS), return_tensors="pt", padding=True)
    assert set(out["goals"]) == {"input_ids", "attention_mask"}
    for k in want:
        assert out["goals"][k].dtype == torch.int64 and torch.equal(out["goals"][k], want[k])
    assert len({int(m.sum()) for m in out["goals"]["attention_mask"]}) > 1          # goals of unequal token length, right-padded
    assert pp.process([]) is None


def test_max_steps_truncates(samples):
    from safevla_amd.il import Preprocessor, PreprocessorConfig

    out = Preprocessor(PreprocessorConfig(max_steps=3), device="cpu").process(samples)
    full = Preprocessor(device="cpu").process(samples)
    assert out["lengths"].tolist() == [3, 2, 1]
    assert torch.equal(out["padding_mask"], torch.arange(3)[None, :] >= torch.tensor([3, 2, 1])[:, None])
    for k in (NAV, MANIP, "actions", "last_actions", "time_ids", "an_object_is_in_hand"):
        assert out[k].shape[:2] == (3, 3) and torch.equal(out[k], full[k][:, :3]), k


def test_custom_goal_key_and_injected_tokenizer(samples):
    from safevla_amd.il import Preprocessor, PreprocessorConfig

    calls = []

    def tok(goals, return_tensors="pt", padding=True):
        calls.append(list(goals))
        return dict(input_ids=torch.full((len(goals), 2), 7), attention_mask=torch.ones(len(goals), 2, dtype=torch.int64))

    out = Preprocessor(PreprocessorConfig(goal_sensor_uuid="natural_language_spec"), device="cpu", tokenizer=tok).process(samples)
    assert calls == [list(GOALS)] and "goals" not in out and out["natural_language_spec"]["input_ids"].tolist() == [[7, 7]] * 3


def test_unknown_action_string_is_a_key_error(samples):
    from safevla_amd.il import Preprocessor

    rs = np.random.RandomState(4)
    bad = _sample(rs, 3, "a goal")
    bad["observations"]["actions"][1] = "moonwalk"
    with pytest.raises(KeyError, match="moonwalk"):
        Preprocessor(device="cpu").process([samples[0], bad])


@pytest.mark.parametrize("key,sensors", [(MANIP, [NAV, "last_actions"]), ("an_object_is_in_hand", [NAV, MANIP, "last_actions"]), ("last_actions", [NAV, MANIP]),
                                         ("nav_task_relevant_object_bbox", None), ("relative_arm_location_metadata", None), ("not_a_sensor", None)])
def test_a_sensor_the_model_is_not_built_for_is_a_value_error(samples, key, sensors):
    from safevla_amd.il import Preprocessor, PreprocessorConfig

    rs = np.random.RandomState(5)
    batch = [_sample(rs, 2, "a goal", extra={key: np.zeros((2, 5), np.float32)} if sensors is None else None)]
    cfg = PreprocessorConfig() if sensors is None else PreprocessorConfig(input_sensors=sensors)
    with pytest.raises(ValueError, match=key):
        Preprocessor(cfg, device="cpu").process(batch)


def test_tokenised_goals_pass_through():
    from safevla_amd.il import Preprocessor, PreprocessorConfig

    rs = np.random.RandomState(6)
    ids = [[917, 4033, 88, 21, 1], [55, 1], [7, 8, 1]]
    batch = [_sample(rs, t, dict(input_ids=torch.tensor(i), attention_mask=np.ones(len(i), np.int64))) for t, i in zip(LENS, ids)]
    goals = Preprocessor(device="cpu", tokenizer=None).process(batch)["goals"]
    assert goals["input_ids"].tolist() == [[917, 4033, 88, 21, 1], [55, 1, 0, 0, 0], [7, 8, 1, 0, 0]]
    assert goals["attention_mask"].tolist() == [[1, 1, 1, 1, 1], [1, 1, 0, 0, 0], [1, 1, 1, 0, 0]]
    # bare ids for a t5 preset: the mask is where the ids are
    bare = Preprocessor(device="cpu").process([_sample(rs, t, np.asarray(i)) for t, i in zip(LENS, ids)])["goals"]
    assert torch.equal(bare["input_ids"], goals["input_ids"]) and torch.equal(bare["attention_mask"], goals["attention_mask"])
    # SigLIP presets: the tokenizer's id rows [64] are stacked; a string goal without a tokenizer is refused (open_clip's is not available offline)
    rows = [np.ones(64, np.int64) * (b + 1) for b in range(3)]
    sig = Preprocessor(PreprocessorConfig(text_encoder="SigLIPBase"), device="cpu")
    out = sig.process([_sample(rs, t, r) for t, r in zip(LENS, rows)])["goals"]
    assert torch.is_tensor(out) and out.dtype == torch.int64 and out.shape == (3, 64) and out[:, 0].tolist() == [1, 2, 3]
    with pytest.raises(ValueError, match="tokenizer"):
        sig.process([_sample(rs, 2, "find a mug")])
