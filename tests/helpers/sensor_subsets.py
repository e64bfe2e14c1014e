"""TEST INFRASTRUCTURE ONLY -- fp32 CPU restatements of the models over a sensor subset, composed from the classes of oracle/ref_model.py and
oracle/ref_il.py, and loaders of the reduced-sensor fixtures (tests/golden/make_golden_sensors.py; pinned by tests/test_sensor_subsets_oracle_cpu.py).

  * ``SubsetTower`` / ``SubsetSafeActorCritic``: ``DinoLLAMATxNavActorCritic`` with ``manipulation_rgb_dino_preprocessor_uuid`` / ``an_object_is_in_hand_uuid``
    that may be None (allenact_dino_transformer.py:67-68,129-132,517-527,663-688): one camera token per camera, no ``object_in_hand_embed`` without the sensor.
    The RL towers always embed the previous action.
  * ``SubsetEarlyFusion``: ``EarlyFusionCnnTransformer`` over ``input_sensors`` (early_fusion_tsfm_models.py:90-102,143-153; text_cond_visual_encoder.py:101-111).
"""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.detfill import _draw, tower_local_name
from oracle.ref_il import MANIP, NAV, RefEarlyFusion
from oracle.ref_model import N_ACTIONS, RefGoalEncoder, RefTower

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
NAV_ACTION_IDS = (0, 1, 2, 3, 4, 6, 7)      # move_ahead, rotate_right, rotate_left, move_back, done, rotate_left_small, rotate_right_small


def _drop_cameras(ve: RefGoalEncoder, cameras):
    for cam in (NAV, MANIP):
        if cam not in cameras:
            delattr(ve, f"visual_sensor_token_{cam}")


class SubsetTower(RefTower):
    def __init__(self, tokenizer, max_steps=500, max_batch=32, dropout=0.0, manip_uuid=None, hand_uuid=None):
        super().__init__(tokenizer, max_steps, max_batch, dropout)
        self.manip_uuid, self.hand_uuid = manip_uuid, hand_uuid
        _drop_cameras(self.visual_encoder, (NAV, MANIP) if manip_uuid is not None else (NAV,))
        if hand_uuid is None:
            del self.object_in_hand_embed

    def _encode(self, obs):
        ve = self.visual_encoder
        nav = obs[ve.nav_uuid]
        T, B = nav.shape[:2]
        R = T * B
        parts = [ve.fusion_token.view(1, 1, -1).expand(R, -1, -1), ve._camera(nav.reshape(R, *nav.shape[-3:]), ve.visual_sensor_token_raw_navigation_camera)]
        if self.manip_uuid is not None:
            parts.append(ve._camera(obs[self.manip_uuid].reshape(R, *nav.shape[-3:]), ve.visual_sensor_token_raw_manipulation_camera))
        parts.append(ve.text_features(obs[ve.goal_uuid].reshape(R, -1)))
        return ve.fusion_xformer(torch.cat(parts, dim=1))[:, 0].view(T, B, -1)

    def tower_forward(self, obs, prev_actions, masks):
        obs_embeds = self._encode(obs)
        T, B = prev_actions.shape
        pa = torch.where(masks.view(T, B) != 0, prev_actions, torch.full_like(prev_actions, N_ACTIONS))
        joint = obs_embeds + self.last_actions_embed(pa)
        if self.hand_uuid is not None:
            joint = joint + self.object_in_hand_embed(obs[self.hand_uuid].squeeze(2))
        if T > 1 or self.time_step_counter >= self.max_steps:
            self.time_step_counter = 0
        joint = self.time_encoder(obs["time_step"]) + joint
        x = joint.permute(1, 0, 2)
        if T == 1:
            start = torch.clamp(self.time_step_counter - obs["time_step"].permute(1, 0), min=0)
            mask = (start <= torch.arange(self.time_step_counter + 1)[None, :])[:, None, None, :]
        else:
            tr = obs["traj_index"].permute(1, 0)
            mask = torch.tril(tr[:, :, None] == tr[:, None, :])[:, None]
        beliefs = self.decoder(x, self.time_step_counter, mask).permute(1, 0, 2)
        if T == 1:
            self.time_step_counter += 1
        return self.actor(beliefs), self.critic(beliefs), beliefs


class SubsetSafeActorCritic(SubsetTower):
    def __init__(self, tokenizer, max_steps=500, max_batch=32, dropout=0.0, manip_uuid=None, hand_uuid=None):
        kw = dict(manip_uuid=manip_uuid, hand_uuid=hand_uuid)
        super().__init__(tokenizer, max_steps, max_batch, dropout, **kw)
        self.critic_tsfm = SubsetTower(tokenizer, max_steps, max_batch, dropout, **kw)
        self.c_critic_tsfm = SubsetTower(tokenizer, max_steps, max_batch, dropout, **kw)

    def forward(self, observations, memory, prev_actions, masks):
        logits, _, _ = self.tower_forward(observations, prev_actions, masks)
        _, values, _ = self.critic_tsfm.tower_forward(observations, prev_actions, masks)
        _, c_values, _ = self.c_critic_tsfm.tower_forward(observations, prev_actions, masks)
        return {"logits": logits, "values": values, "c_values": c_values}, memory


class SubsetEarlyFusion(RefEarlyFusion):
    def __init__(self, input_sensors, **kw):
        super().__init__(**kw)
        self.input_sensors = list(input_sensors)
        self.cameras = sorted(s for s in self.input_sensors if s in (NAV, MANIP))      # sensors in sorted order (text_cond_visual_encoder.py:105)
        _drop_cameras(self.visual_encoder, self.cameras)
        if "last_actions" not in self.input_sensors:
            del self.last_actions_embed
        if "an_object_is_in_hand" not in self.input_sensors:
            del self.object_in_hand_embed

    def encode(self, batch):
        ve = self.visual_encoder
        first = batch[self.cameras[0]]
        B, T = first.shape[:2]
        R = B * T
        with torch.no_grad():
            text = ve.text_encoder(batch["goals"]["input_ids"], batch["goals"]["attention_mask"])
        text = ve.text_adapter(text)
        parts = [ve.fusion_token.view(1, 1, -1).expand(R, -1, -1)]
        for key in self.cameras:
            parts.append(ve._camera(batch[key].reshape(R, *first.shape[-3:]), getattr(ve, f"visual_sensor_token_{key}")))
        parts.append(text.unsqueeze(1).expand(B, T, -1, -1).reshape(R, text.shape[1], -1))
        return ve.fusion_xformer(torch.cat(parts, dim=1))[:, 0].view(B, T, -1)

    def forward(self, batch):
        x = self.encode(batch)
        if "last_actions" in self.input_sensors:
            x = x + self.last_actions_embed(batch["last_actions"])
        if "an_object_is_in_hand" in self.input_sensors:
            x = x + self.object_in_hand_embed(batch["an_object_is_in_hand"])
        x = x + self.time_encoder(batch["time_ids"])
        B, T = x.shape[:2]
        mask = torch.tril(torch.ones(T, T, dtype=torch.bool))[None, None].expand(B, 1, T, T)
        logits = self.actor(self.decoder(x, 0, mask))
        loss = F.cross_entropy(logits.reshape(-1, N_ACTIONS), batch["actions"].reshape(-1), ignore_index=-1)
        return dict(actions_logits=logits, actions_loss=loss, loss=loss)


# ---- weights ---------------------------------------------------------------------------------------------------------------------------------------
def fill_towers_alike(module: nn.Module, seed: int = 7, skip=("div_term",)) -> None:
    """``oracle.detfill.fill_state_dict`` with EVERY tensor drawn by its tower-local name: the three towers of a model then hold the weights of the one
    reference tower behind fixture (a), so its logits (actor tower) and values (either critic tower) are that tower's."""
    with torch.no_grad():
        for name, t in module.state_dict().items():
            if any(s in name for s in skip) or not t.dtype.is_floating_point:
                continue
            key = tower_local_name(name).replace("encoder.embed_tokens.weight", "shared.weight")
            t.copy_(torch.from_numpy(_draw(key, tuple(t.shape), seed)).to(t.device))


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------------------------
def _npz(name):
    return dict(np.load(os.path.join(GOLDEN, name), allow_pickle=False))


_CACHE = {}


def load_rl_nav():
    """fixture (a) -> (g, update observations, acting observations); the navigation camera's features are the float16-rounded ``obs:rgb_dinov2`` of
    g5_mixedlen.npz, its first 6 x 2 (update) and 7 x 4 (acting) blocks.  Loaded once; callers leave the arrays unchanged."""
    if "rl" not in _CACHE:
        g = _npz("s1_rl_nav.npz")
        feat = _npz("g5_mixedlen.npz")["obs:rgb_dinov2"].astype(np.float16).astype(np.float32)
        T, B = g["prev_actions"].shape
        n, E = g["act:prev_actions"].shape
        upd = {k[4:]: v for k, v in g.items() if k.startswith("obs:")}
        upd["rgb_dinov2"] = np.ascontiguousarray(feat[:T, :B])
        act = {k[4:]: v for k, v in g.items() if k.startswith("act:") and k[4:] not in ("prev_actions", "masks", "logits", "values")}
        act["rgb_dinov2"] = np.ascontiguousarray(feat[:n, :E])
        _CACHE["rl"] = (g, upd, act)
    return _CACHE["rl"]


def load_il(tag):
    """fixture (b) ``s2_il_cameras`` / (c) ``s3_il_nav_last`` -> (g, batch as numpy arrays holding the fixture's sensors only); the batch is g8_il.npz's"""
    if tag not in _CACHE:
        g, g8 = _npz(tag + ".npz"), _npz("g8_il.npz")
        sensors = [str(s) for s in g["input_sensors"]]
        batch = {k: (g8[k].astype(np.float32) if g8[k].dtype == np.float16 else g8[k]) for k in sensors + ["time_ids", "actions", "padding_mask"]}
        batch["goals"] = dict(input_ids=g8["goal_ids"], attention_mask=g8["goal_mask"])
        _CACHE[tag] = (g, sensors, batch)
    return _CACHE[tag]


def to_torch(d, device=None):
    out = {}
    for k, v in d.items():
        out[k] = to_torch(v, device) if isinstance(v, dict) else (torch.from_numpy(v) if device is None else torch.from_numpy(v).to(device))
    return out


def manifest(name):
    return {l.split("\t")[0]: l.rstrip("\n").split("\t")[1] for l in open(os.path.join(GOLDEN, name))}
