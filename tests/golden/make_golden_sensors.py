#!/usr/bin/env python3
"""Golden vectors of the reduced sensor sets, produced by the REFERENCE ITSELF (build container only; shims of make_golden.py / make_golden_il.py).

    python tests/golden/make_golden_sensors.py        # writes tests/golden/s1_*.npz, s2_*.npz, s3_*.npz and their name manifests

  (a) s1_rl_nav.npz          one ``DinoLLAMATxNavActorCritic`` in the navigation-only configuration of ``DinoV2ViTSTSFMBaseParams.full_sensor = False``
                             (manipulation_rgb_dino_preprocessor_uuid = an_object_is_in_hand_uuid = None): an update pass T = 6, B = 2 (goals of two token
                             lengths, two trajectories in env column 0) with logits, values and gradient checksums, and 7 KV-cached acting steps x 4 envs.
  (b) s2_il_cameras.npz      IL ``small_3`` with input_sensors = [raw_navigation_camera, raw_manipulation_camera] (the reference trainer's default)
  (c) s3_il_nav_last.npz     IL ``small_3`` with input_sensors = [raw_navigation_camera, last_actions]

Inputs are not stored twice: the camera features come from fixtures that are already tracked -- (a) reads ``obs:rgb_dinov2`` of g5_mixedlen.npz (the first
6 x 2 resp. 7 x 4 blocks, rounded to float16 as g8 stores its features), (b) and (c) read the batch of g8_il.npz (B = 2, T = 8, one row padded).  The new
files hold the remaining inputs (time steps, trajectories, goals, previous actions, loss weights) and the reference's outputs.  Weights on both sides are
name-seeded (oracle.detfill), every tower-local name drawn alike, so a fixture holds no parameters."""
import importlib
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from oracle.detfill import fill_state_dict, grad_probe  # noqa: E402

UPDATE_GOALS = ["find a mug", "navigate to the red apple", "fetch the small blue vase now"]       # 4, 6 and 8 tokens (<= 9)
ACTING_GOALS = ["find a mug", "navigate to the red apple", "go to sofa", "pick up a bowl"]        # 4, 6, 4 and 5 tokens


def f16(x):
    return x.astype(np.float16).astype(np.float32)


def rl_inputs():
    """The navigation-only fixture's inputs, rebuilt identically by the tests (tests/helpers/sensor_subsets.py reads them from the fixture)."""
    from safevla_amd.text import str_to_bytes

    feat = f16(dict(np.load(os.path.join(HERE, "g5_mixedlen.npz"), allow_pickle=False))["obs:rgb_dinov2"])      # [8, 4, 384, 7, 12]
    rs = np.random.RandomState(41)
    T, B = 6, 2
    goal = np.zeros((T, B, 1000), np.uint8)
    # env column 0: trajectory 11 (goal 0) for three steps, then trajectory 12 (goal 1: another token length) from time step 0; column 1: one trajectory in progress
    time_step = np.array([[7, 17], [8, 18], [9, 19], [0, 20], [1, 21], [2, 22]], np.int64)
    traj = np.array([[11, 5], [11, 5], [11, 5], [12, 5], [12, 5], [12, 5]], np.int64)
    masks = np.ones((T, B, 1), np.float32)
    masks[0, :, 0] = 0.0
    masks[3, 0, 0] = 0.0
    for t in range(T):
        goal[t, 0] = str_to_bytes(UPDATE_GOALS[0 if t < 3 else 1])[:1000]
        goal[t, 1] = str_to_bytes(UPDATE_GOALS[2])[:1000]
    upd = {"obs:rgb_dinov2": np.ascontiguousarray(feat[:T, :B]), "obs:time_step": time_step, "obs:traj_index": traj, "obs:natural_language_spec": goal,
           "prev_actions": rs.randint(0, 20, size=(T, B)).astype(np.int64), "masks": masks,
           "w_logits": rs.standard_normal((T, B, 20)).astype(np.float32), "w_values": rs.standard_normal((T, B, 1)).astype(np.float32)}
    n, E = 7, 4
    a_goal = np.zeros((n, E, 1000), np.uint8)
    # env 0 starts an episode with the rollout; env 1 restarts at step 3 (new goal of the same length); env 2 is 5 steps into its episode; env 3 restarts at step 5
    a_ts = np.array([[0, 0, 5, 2], [1, 1, 6, 3], [2, 2, 7, 4], [3, 0, 8, 5], [4, 1, 9, 6], [5, 2, 10, 0], [6, 3, 11, 1]], np.int64)
    a_masks = np.ones((n, E, 1), np.float32)
    a_masks[0, :, 0] = 0.0
    a_masks[3, 1, 0] = 0.0
    a_masks[5, 3, 0] = 0.0
    for t in range(n):
        for e in range(E):
            g = ACTING_GOALS[e]
            if e == 1 and t >= 3:
                g = ACTING_GOALS[0]
            a_goal[t, e] = str_to_bytes(g)[:1000]
    act = {"act:rgb_dinov2": np.ascontiguousarray(feat[:n, :E]), "act:time_step": a_ts, "act:traj_index": np.cumsum(a_masks[:, :, 0] == 0, axis=0).astype(np.int64) + 100 * np.arange(E)[None, :],
           "act:natural_language_spec": a_goal, "act:prev_actions": rs.randint(0, 20, size=(n, E)).astype(np.int64), "act:masks": a_masks}
    return upd, act


def main_rl():
    import make_golden as mg

    gym, SpaceDict, Box, Discrete = mg.install_shims()
    from transformers import T5Config, T5EncoderModel

    from safevla_amd.text import GoalTokenizer

    class _T5:
        @staticmethod
        def from_pretrained(name):
            return T5EncoderModel(T5Config(vocab_size=32128, d_model=512, d_kv=64, d_ff=2048, num_layers=6, num_heads=8, feed_forward_proj="relu"))

    class _Tok:
        @staticmethod
        def from_pretrained(name):
            return GoalTokenizer()

    adt = importlib.import_module("architecture.models.allenact_transformer_models.allenact_dino_transformer")
    adt.T5EncoderModel, adt.AutoTokenizer = _T5, _Tok
    obs_space = SpaceDict({"rgb_dinov2": Box(shape=(7, 12, 384)), "natural_language_spec": Box(shape=(1000,)), "time_step": Box(), "traj_index": Box()})
    torch.manual_seed(0)
    torch.set_num_threads(8)
    # dinov2_vits_tsfm_base.py:227-270 with full_sensor = False
    model = adt.DinoLLAMATxNavActorCritic(
        action_space=Discrete(20), observation_space=obs_space, goal_sensor_uuid="natural_language_spec", rgb_dino_preprocessor_uuid="rgb_dinov2",
        manipulation_rgb_dino_preprocessor_uuid=None, an_object_is_in_hand_uuid=None, num_tx_layers=3, num_tx_heads=8, hidden_size=512, goal_dims=512,
        add_prev_actions=True, add_prev_action_null_token=True, auxiliary_uuids=[], max_steps=500, time_step_uuid="time_step",
        initial_tgt_cache_shape=(500, 4, 512), traj_idx_uuid="traj_index", traj_max_idx=2048, relevant_object_box_uuid=None, accurate_object_box_uuid=None,
        prev_checkpoint=None)
    model.eval()
    fill_state_dict(model, seed=7)
    with open(os.path.join(HERE, "state_dict_manifest_rl_nav.txt"), "w") as f:
        for k, v in model.state_dict().items():
            f.write(f"{k}\t{tuple(v.shape)}\n")
    upd, act = rl_inputs()
    obs = {k[4:]: torch.from_numpy(v) for k, v in upd.items() if k.startswith("obs:")}
    for p in model.parameters():
        p.grad = None
    aco, _ = model(obs, None, torch.from_numpy(upd["prev_actions"]), torch.from_numpy(upd["masks"]))
    logits = aco.distributions.logits                              # normalised (Categorical)
    ((logits * torch.from_numpy(upd["w_logits"])).sum() + (aco.values * torch.from_numpy(upd["w_values"])).sum()).backward()
    out = {k: v for k, v in upd.items() if k != "obs:rgb_dinov2"}
    out.update(logits=logits.detach().numpy(), values=aco.values.detach().numpy())
    names = []
    for n, p in model.named_parameters():
        if p.grad is not None and float(p.grad.abs().sum()) > 0:
            out["gp:" + n] = np.array(grad_probe(n, p.grad), np.float64)
            names.append(n)
    out["grad_names"] = np.array(names)
    model.time_step_counter = 0
    lg, vs = [], []
    with torch.no_grad():
        for t in range(act["act:masks"].shape[0]):
            o = {k[4:]: torch.from_numpy(v[t:t + 1]) for k, v in act.items() if k not in ("act:prev_actions", "act:masks")}
            a, _ = model(o, None, torch.from_numpy(act["act:prev_actions"][t:t + 1]), torch.from_numpy(act["act:masks"][t:t + 1]))
            lg.append(a.distributions.logits.numpy()); vs.append(a.values.numpy())
    out.update({k: v for k, v in act.items() if k != "act:rgb_dinov2"})
    out.update({"act:logits": np.concatenate(lg), "act:values": np.concatenate(vs)})
    np.savez_compressed(os.path.join(HERE, "s1_rl_nav.npz"), **out)
    print("wrote s1_rl_nav.npz:", len(names), "trained tensors with gradient;", len(model.state_dict()), "state_dict names")


def main_il():
    import make_golden_il as mi

    mi.install()
    from transformers import T5Config, T5EncoderModel

    class _T5:
        @staticmethod
        def from_pretrained(name):
            return T5EncoderModel(T5Config(vocab_size=32128, d_model=512, d_kv=64, d_ff=2048, num_layers=6, num_heads=8, feed_forward_proj="relu"))

    tc = importlib.import_module("architecture.models.transformer_models.text_cond_visual_encoder")
    tc.T5EncoderModel = _T5
    ef = importlib.import_module("architecture.models.transformer_models.early_fusion_tsfm_models")
    g8 = dict(np.load(os.path.join(HERE, "g8_il.npz"), allow_pickle=False))
    torch.set_num_threads(8)
    for tag, sensors in (("s2_il_cameras", ["raw_navigation_camera", "raw_manipulation_camera"]), ("s3_il_nav_last", ["raw_navigation_camera", "last_actions"])):
        cfg = ef.EarlyFusionCnnTransformerConfig()
        cfg.visual_encoder = tc.TextCondVisualEncoderConfig()
        cfg.visual_encoder.input_sensors = list(sensors)
        cfg.decoder = tc.TransformerConfig(3, 512, 8)
        torch.manual_seed(0)
        model = ef.EarlyFusionCnnTransformer(cfg).eval()
        fill_state_dict(model, seed=7, share_t5=False)
        # forward(batch) sorts the batch into visual / non-visual sensors by name (early_fusion_tsfm_models.py:185-190): the batch holds the model's sensors only
        keys = [k for k in sensors] + ["time_ids", "actions", "padding_mask"]
        tb = {k: torch.from_numpy(g8[k].astype(np.float32) if g8[k].dtype == np.float16 else g8[k]) for k in keys}
        tb["goals"] = dict(input_ids=torch.from_numpy(g8["goal_ids"]), attention_mask=torch.from_numpy(g8["goal_mask"]))
        for p in model.parameters():
            p.grad = None
        out = model(tb)
        out["loss"].backward()
        g = dict(input_sensors=np.array(sensors), logits=out["actions_logits"].detach().numpy(), loss=np.float64(out["loss"].item()))
        n = 0
        for name, p in model.named_parameters():
            if p.grad is not None and "text_encoder" not in name:
                g["gp:" + name] = np.array(grad_probe(name, p.grad), np.float64)
                n += 1
        np.savez_compressed(os.path.join(HERE, tag + ".npz"), **g)
        with open(os.path.join(HERE, f"state_dict_manifest_{tag}.txt"), "w") as f:
            for k, v in model.state_dict().items():
                f.write(f"{k}\t{tuple(v.shape)}\n")
        print(f"wrote {tag}.npz: loss", out["loss"].item(), "trained tensors", n)


if __name__ == "__main__":
    if len(sys.argv) > 1:
        {"rl": main_rl, "il": main_il}[sys.argv[1]]()
    else:       # the two shim sets replace the same module names: one process each
        for part in ("rl", "il"):
            subprocess.run([sys.executable, os.path.abspath(__file__), part], check=True)
