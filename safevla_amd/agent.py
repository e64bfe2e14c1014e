"""Evaluation / rollout-time agent on the MI355X acting path.

Mirrors ``InferenceAgentVIDA`` (/root/reference/architecture/models/allenact_transformer_models/inference_agent.py:74-296) behind
``AbstractAgent`` (/root/reference/architecture/agent.py:5-51): ``reset()``, ``get_action_list()`` and
``get_action(frame, goal_spec) -> (action_str, action_probs)``.  One call = uint8 frames -> frozen DINOv2 ViT preprocessor
(``preproc.DinoViTPreprocessor``) -> single-step 3-tower forward with per-tower llama KV caches (``model`` acting path) ->
sample / mode.  The rollout storage is used exactly as the reference uses it (``initialize`` on the first step of a task, ``add``
with dummy value/reward fields afterwards, ``agent_input_for_next_step``), so the prev-action / mask / time-step plumbing is the
update path's own.

``VectorInferenceAgentVIDA`` (``InferenceAgentVIDA.build_vector_agent``) serves many such episodes at once behind one set of weights: actor tower only, per-row KV
rings, one-launch sampling.
"""
import json
import os
import warnings
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import checkpoint
from .preproc import DinoViTPreprocessor
from .storage import RolloutStorage
from .text import str_to_bytes
from .vector_slots import EpisodeSlots, goal_ids, restart_slot

# Stretch action vocabulary in the order of the policy head (utils/constants/stretch_initialization_utils.py:145-166,
# short names utils/type_utils.py:55-74; the ACTION_DICT / LONG_ACTION_NAME environment overrides are honoured like upstream)
ALL_STRETCH_ACTIONS = ["m", "r", "l", "b", "end", "sub_done", "ls", "rs", "p", "zm", "zp", "yp", "ym", "wp", "wm", "yms", "zms",
                       "zps", "yps", "d"]
STRETCH_LONG_NAMES = {"m": "move_ahead", "r": "rotate_right", "l": "rotate_left", "b": "move_back", "end": "done",
                      "sub_done": "sub_done", "ls": "rotate_left_small", "rs": "rotate_right_small", "p": "pickup",
                      "zm": "move_arm_in", "zp": "move_arm_out", "yp": "move_arm_up", "ym": "move_arm_down", "wp": "wrist_open",
                      "wm": "wrist_close", "yms": "move_arm_down_small", "zms": "move_arm_in_small", "zps": "move_arm_out_small",
                      "yps": "move_arm_up_small", "d": "dropoff"}
# what a navigation-only policy may choose (dinov2_vits_tsfm_base.py:272-289): move_ahead, rotate_right, rotate_left, move_back, done, rotate_right_small, rotate_left_small
NAV_ACTIONS = ("m", "r", "l", "b", "end", "rs", "ls")


def camera_preprocessors(uuids, device, nav_pre=None, manip_pre=None):
    """-> (nav_pre, manip_pre): the frozen ViT fronts of the two cameras' raw frames, built where none was passed in.  One frozen ViT serves both cameras only when
    neither was passed in; a policy without the manipulation camera (manipulation_rgb_dino_preprocessor_uuid=None) gets no preprocessor for it"""
    shared = nav_pre is None and manip_pre is None
    nav_pre = nav_pre or DinoViTPreprocessor("rgb_raw", uuids["nav"], device=device)
    manip_pre = None if uuids["manip"] is None else (manip_pre or DinoViTPreprocessor("manipulation_rgb_raw", uuids["manip"], device=device))
    if shared and manip_pre is not None:
        manip_pre.vit = nav_pre.vit
    return nav_pre, manip_pre


class AbstractAgent:
    def reset(self) -> None:
        raise NotImplementedError

    def get_action_list(self) -> List[str]:
        raise NotImplementedError

    def get_action(self, observations: Dict[str, Any], goal: str) -> Tuple[str, Any]:
        raise NotImplementedError


class InferenceAgentVIDA(AbstractAgent):
    num_evaluated_traj = 0

    def __init__(self, actor_critic, device="cuda", greedy_sampling: bool = False, nav_preprocessor=None, manip_preprocessor=None,
                 steps_before_rollout_refresh: int = 64, generator: Optional[torch.Generator] = None):
        self.actor_critic = actor_critic
        self.device = torch.device(device)
        self.greedy_sampling = greedy_sampling
        u = actor_critic.uuids
        self.nav_pre, self.manip_pre = camera_preprocessors(u, device, nav_preprocessor, manip_preprocessor)
        self.steps_before_rollout_refresh = steps_before_rollout_refresh
        self.rollout_storage = RolloutStorage(steps_before_rollout_refresh, device=device, store_tokens=True,
                                              nav_uuid=u["nav"], manip_uuid=u["manip"])
        self.generator = generator
        self.has_initialized = False
        self.memory = None
        self.steps_taken_in_task = 0
        self.last_action_flat = None

    IL_VIT_PREFIX = "model.visual_encoder.image_encoder.model."      # where a Lightning IL checkpoint keeps its DINOv2 weights

    @classmethod
    def build_agent(cls, actor_critic, device="cuda", greedy_sampling: bool = False, ckpt_path: Optional[str] = None,
                    spiece_model: Optional[str] = None, vit_weights: Optional[str] = None, **kw):
        """ckpt formats auto-detected like upstream (:128-165): Lightning ``state_dict`` (IL), AllenAct ``model_state_dict``, or a
        bare state dict.

        The reference pulls two more assets from the network that a checkpoint does not (or only partly) contain: the ``t5-small``
        sentencepiece vocabulary and the frozen DINOv2 ViT-S/14 weights (torch.hub).  ``spiece_model`` = path of ``spiece.model``;
        ``vit_weights`` = path of a DINOv2 ViT-S/14 ``state_dict`` (hub names).  A Lightning IL checkpoint that carries its image
        encoder (``model.visual_encoder.image_encoder.model.*``) fills the ViT from there.  Running real weights on the offline
        stand-ins (word-hash token ids, random-init ViT) produces meaningless actions, so that combination WARNS loudly."""
        vit_sd = cls._load_assets(actor_critic, ckpt_path, spiece_model, vit_weights)
        agent = cls(actor_critic, device=device, greedy_sampling=greedy_sampling, **kw)
        cls._load_vit(agent, vit_sd)
        cls._warn_stand_ins(actor_critic, ckpt_path, vit_sd, kw)
        agent.reset()
        return agent

    @classmethod
    def build_vector_agent(cls, actor_critic, num_episodes: int = 1, device="cuda", greedy_sampling: bool = False, ckpt_path: Optional[str] = None,
                           spiece_model: Optional[str] = None, vit_weights: Optional[str] = None, **kw):
        """The same policy behind ``VectorInferenceAgentVIDA``: ``num_episodes`` evaluation episodes served by one set of weights, the actor tower only.  Checkpoint,
        ``spiece_model`` and ``vit_weights`` as in ``build_agent``; ``kw``: ``seed``, ``nav_preprocessor``, ``manip_preprocessor``."""
        vit_sd = cls._load_assets(actor_critic, ckpt_path, spiece_model, vit_weights)
        agent = VectorInferenceAgentVIDA(actor_critic, num_episodes, device=device, greedy_sampling=greedy_sampling, **kw)
        if vit_sd is not None:                  # (without weights to load the frozen ViT is built by the first raw frame: pre-encoded features need none)
            agent._preprocessors()
            cls._load_vit(agent, vit_sd)
        cls._warn_stand_ins(actor_critic, ckpt_path, vit_sd, kw)
        return agent

    # ---- what build_agent and build_vector_agent share ------------------------------------------------------------------------------
    @classmethod
    def _load_assets(cls, actor_critic, ckpt_path, spiece_model, vit_weights):
        """checkpoint -> the policy, ``spiece_model`` -> its tokenizer, eval mode; -> the state dict for the frozen ViT (from the checkpoint or ``vit_weights``) or None"""
        vit_sd = None
        if ckpt_path is not None:
            ckpt = torch.load(ckpt_path, map_location="cpu")
            if "state_dict" in ckpt:
                checkpoint.load_pl_ckpt_allenact(actor_critic, ckpt)
                actor_critic.sync_weights()
                vit_sd = {k[len(cls.IL_VIT_PREFIX):]: v for k, v in ckpt["state_dict"].items() if k.startswith(cls.IL_VIT_PREFIX)} or None
            elif "model_state_dict" in ckpt:
                actor_critic.load_state_dict(ckpt["model_state_dict"], strict=False)
            elif any(k.startswith(("visual_encoder.", "actor.", "decoder.")) for k in ckpt):
                actor_critic.load_state_dict(ckpt, strict=False)
            else:
                raise ValueError(f"Unknown checkpoint format; found keys {list(ckpt.keys())[:10]}")
        if spiece_model is not None:
            from .text import GoalTokenizer

            actor_critic.tokenizer = GoalTokenizer(spiece_model)
            actor_critic._goal_cache.clear()
        if vit_weights is not None:
            vit_sd = torch.load(vit_weights, map_location="cpu")
        actor_critic.eval()     # AllenAct's InferenceAgent runs the policy in eval mode (mode="test", inference_agent.py:98-102)
        return vit_sd

    @staticmethod
    def _load_vit(agent, vit_sd):
        if vit_sd is None:
            return
        missing, unexpected = agent.nav_pre.vit.load_state_dict(vit_sd, strict=False)
        if missing:
            warnings.warn(f"DINOv2 weights: {len(missing)} tensors not found (e.g. {missing[:3]}); those stay random-init")
        agent.nav_pre.vit.sync()
        if agent.manip_pre is not None and agent.manip_pre.vit is not agent.nav_pre.vit:
            agent.manip_pre.vit.load_state_dict(vit_sd, strict=False)
            agent.manip_pre.vit.sync()

    @staticmethod
    def _warn_stand_ins(actor_critic, ckpt_path, vit_sd, kw):
        if ckpt_path is None:
            return
        stand_ins = []
        if getattr(actor_critic.tokenizer, "_sp", None) is None:
            stand_ins.append("word-hash goal tokenizer (pass spiece_model=<t5-small spiece.model>)")
        if vit_sd is None and kw.get("nav_preprocessor") is None:
            stand_ins.append("random-init DINOv2 ViT (pass vit_weights=<dinov2_vits14 state_dict>)")
        if stand_ins:
            warnings.warn("checkpoint loaded but offline stand-ins are active: " + "; ".join(stand_ins) +
                          " -- the policy's inputs do not match what it was trained on, actions are meaningless", RuntimeWarning)

    # ---- AbstractAgent ------------------------------------------------------------------------------------------------------
    def reset(self):
        if self.has_initialized:
            self.rollout_storage.after_updates()
        self.steps_taken_in_task = 0
        type(self).num_evaluated_traj += 1
        self.traj_index = type(self).num_evaluated_traj
        self.memory = None

    def get_action_list(self) -> List[str]:
        if os.getenv("ACTION_DICT") is not None:
            return list(json.load(open(os.getenv("ACTION_DICT"), "r")).keys())
        if os.getenv("LONG_ACTION_NAME") is not None and bool(int(os.getenv("LONG_ACTION_NAME"))):
            return [STRETCH_LONG_NAMES[a] for a in ALL_STRETCH_ACTIONS]
        return list(ALL_STRETCH_ACTIONS)

    def get_action(self, frame: Dict[str, Any], goal_spec: str) -> Tuple[str, torch.Tensor]:
        """frame: the evaluator's sensor dict (``raw_navigation_camera`` [, ``raw_manipulation_camera``, ``an_object_is_in_hand``])."""
        optional = {"raw_manipulation_camera": "manipulation_rgb_raw", "an_object_is_in_hand": "an_object_is_in_hand"}
        sensors = {dst: frame[src] for src, dst in optional.items() if src in frame}
        sensors.update(rgb_raw=frame["raw_navigation_camera"], natural_language_spec=str_to_bytes(goal_spec, 1000),
                       time_step=self.steps_taken_in_task, traj_index=self.traj_index)
        return self.act(sensors, goal_spec)

    # ---- one acting step ----------------------------------------------------------------------------------------------------
    def _batch(self, observations: Dict[str, Any]) -> Dict[str, torch.Tensor]:
        dev, u = self.device, self.actor_critic.uuids
        as_u8 = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev).reshape((1,) + tuple(np.shape(a)))
        nav = as_u8(observations["rgb_raw"])
        batch = {
            u["nav"]: self.nav_pre.process({"rgb_raw": nav}),
            u["goal"]: torch.as_tensor(np.asarray(observations["natural_language_spec"], dtype=np.uint8)).to(dev).reshape(1, -1),
            u["time"]: torch.tensor([int(observations["time_step"])], device=dev, dtype=torch.int64),
            u["traj"]: torch.tensor([int(observations["traj_index"])], device=dev, dtype=torch.int64),
        }
        if self.manip_pre is not None:
            manip = as_u8(observations["manipulation_rgb_raw"]) if "manipulation_rgb_raw" in observations else torch.zeros_like(nav)
            batch[u["manip"]] = self.manip_pre.process({"manipulation_rgb_raw": manip})
        if u["hand"] is not None:      # a policy without the in-hand sensor reads no such observation
            batch[u["hand"]] = torch.tensor([int(np.asarray(observations.get("an_object_is_in_hand", 0)).reshape(-1)[0])], device=dev, dtype=torch.int64)
        return batch

    def _remember(self, obs_batch: Dict[str, torch.Tensor]):
        """Feed the step's observations to the rollout storage the way the update path's storage is fed: a task's first step
        (re)initialises it, later steps append with the sampled previous action; value / reward / cost fields are unused placeholders."""
        st = self.rollout_storage
        if self.steps_taken_in_task > 0:
            zero = torch.zeros((1, 1), device=self.device)
            st.add(observations=obs_batch, memory=self.memory, actions=self.last_action_flat, action_log_probs=zero, value_preds=zero,
                   rewards=zero, costs=zero, c_value_preds=zero, masks=torch.ones((1, 1), device=self.device))   # one task until reset(): never "done"
            return
        self.has_initialized = True
        st.initialize(observations=obs_batch, num_samplers=1, recurrent_memory_specification=self.actor_critic.recurrent_memory_specification,
                      action_space=None)
        st.after_updates()

    @torch.no_grad()
    def act(self, observations: Dict[str, Any], goal_spec: str = "") -> Tuple[str, torch.Tensor]:
        self._remember(self._batch(observations))
        st = self.rollout_storage
        out, self.memory = self.actor_critic(**st.agent_input_for_next_step())
        dist = out.distributions
        sampled, greedy = dist.sample(generator=self.generator), dist.mode()
        self.last_action_flat = sampled.reshape(1)          # what the policy sees as "previous action" next step is the sampled action, also when acting greedily
        self.steps_taken_in_task += 1
        if st.step == st.T:                                 # storage full: roll the last slot to the front
            st.after_updates()
        idx = int((greedy if self.greedy_sampling else sampled).reshape(-1)[0])
        return self.get_action_list()[idx], dist.probs[0][0]


class VectorInferenceAgentVIDA:
    """``num_episodes`` online evaluation episodes of the RL policy behind one set of weights: what ``InferenceAgentVIDA`` does for one episode, for a vector of
    them that start, end and stall independently -- the evaluation workers of the reference (online_evaluation/) hold one model copy each.  ``reset(slot, goal_spec)``
    starts an episode in a slot; ``get_actions({slot: frame})`` steps any non-empty subset of the started slots as ONE compact batch and returns
    ``{slot: (action_str, action_probs[20])}``; slots that are absent keep their cache and their age.

    Only the actor tower runs (``Tower.run_forward`` on the policy itself): evaluation reads the action distribution alone, so ``critic_tsfm`` and ``c_critic_tsfm`` --
    two thirds of a single agent's step -- are never launched.  bf16 only, eval mode.

    Per row the policy sees what ``InferenceAgentVIDA`` feeds it: ``time_step`` = the slot's age, the previous action = the action SAMPLED at the slot's last step (also
    when acting greedily), ``masks`` = 0 on the slot's first step and 1 afterwards, the in-hand sensor and the manipulation camera only if the model has them.  A frame
    carries raw uint8 camera frames under the evaluator's names (``raw_navigation_camera`` [, ``raw_manipulation_camera``]; one batched pass of the frozen ViT per
    camera and call) or already-encoded features [384, 7, 12] under the model's own ``uuids["nav"]`` / ``uuids["manip"]``; ``an_object_is_in_hand`` as the single agent.

    Slot s owns row s of the actor tower's llama KV caches, a ring of W = ``actor_critic.max_steps`` slots.  The RL reference has no sliding window: it restarts its
    cache when its step counter reaches ``max_steps`` (allenact_dino_transformer.py:376-377), so a step of age a writes ring slot a % W and reads the a % W + 1 first
    slots; an episode that reaches W steps restarts its window (one warning per agent, as the single agents warn) while ``time_step`` keeps counting.  Goals of
    different lengths are right-padded to the longest; the padding is masked in T5 and hidden from every fusion layer (``Prep.fusion_kvalid``), and the action is
    drawn by ``ops.policy_sample_rows`` from a counter (seed, slot, age) -- an episode's probabilities and sampled actions do not depend on which other slots share
    its batch.  The frozen T5 reruns only when a ``reset`` brought a different goal.

    One kind of agent on a model at a time: the cache rows are the tower's own, shared with the single agent and the rollout path (which write row 0 ... B - 1 at the
    tower's step counter), so stepping either in between overwrites the slots' histories.  The tower's step counter is neither read nor advanced here; when the vector
    agent has to reallocate the caches, every recorded acting plan is dropped (``invalidate_recorded``)."""

    RAW_CAMERAS = ("raw_navigation_camera", "raw_manipulation_camera")        # evaluator's names of the raw frames -> the inputs of nav_pre / manip_pre
    _PRE_INPUTS = ("rgb_raw", "manipulation_rgb_raw")

    def __init__(self, actor_critic, num_episodes: int, device="cuda", greedy_sampling: bool = False, nav_preprocessor=None, manip_preprocessor=None, seed: int = 0):
        from .model import BF16
        self._slots = EpisodeSlots(num_episodes, 0)            # last action: the action sampled at the slot's last step
        if actor_critic.adt != BF16:
            raise NotImplementedError("precision='fp32': the acting step on per-row KV rings exists on the bf16 product path only")
        self.actor_critic, self.device, self.greedy_sampling = actor_critic, torch.device(device), greedy_sampling
        self.num_episodes, self.seed = self._slots.num_episodes, int(seed)
        self.window = actor_critic.max_steps
        self.nav_pre, self.manip_pre = nav_preprocessor, manip_preprocessor
        self._warned_window = False
        actor_critic.eval()

    get_action_list = InferenceAgentVIDA.get_action_list

    def _preprocessors(self):
        """the frozen ViT front of raw frames, built on first use (pre-encoded features never need it); one ViT serves both cameras, as in ``InferenceAgentVIDA``"""
        self.nav_pre, self.manip_pre = camera_preprocessors(self.actor_critic.uuids, self.device, self.nav_pre, self.manip_pre)

    def age(self, slot: int) -> int:
        return self._slots.age(slot)

    def reset(self, slot: int, goal_spec):
        """Start an episode in ``slot``.  ``goal_spec``: a string (tokenised here, once, with ``actor_critic.tokenizer``) or token ids -- ``{"input_ids"[,
        "attention_mask"]}`` or an id sequence; right-padded ids keep their tokens"""
        slot = self._slots.slot(slot)
        ids = goal_ids(self.actor_critic.tokenizer.encode(goal_spec) if isinstance(goal_spec, str) else goal_spec)
        if not ids:                                              # this agent only: the IL vector agent takes an empty goal as it comes
            raise ValueError("an empty goal")
        self._slots.start(slot, ids)

    def _features(self, obs, cam: int) -> torch.Tensor:
        """camera ``cam`` of the call's frames -> features [n, 384, 7, 12] fp32: pre-encoded ones as they come, raw uint8 frames through ONE batched pass of the ViT"""
        u, dev = self.actor_critic.uuids, self.device
        feat_key, raw_key = (u["nav"], u["manip"])[cam], self.RAW_CAMERAS[cam]
        stack = lambda key: torch.stack([o[key] if torch.is_tensor(o[key]) else torch.as_tensor(np.ascontiguousarray(o[key])) for o in obs]).to(dev)
        if all(feat_key in o for o in obs):
            return stack(feat_key).float()
        self._preprocessors()
        if cam == 1 and not all(raw_key in o for o in obs):      # a policy with the manipulation camera, an evaluator without: black frames, as the single agent
            like = np.asarray(obs[0][self.RAW_CAMERAS[0]])
            obs = [o if raw_key in o else {raw_key: np.zeros_like(like)} for o in obs]
        return (self.nav_pre, self.manip_pre)[cam].process({self._PRE_INPUTS[cam]: stack(raw_key)})

    @torch.no_grad()
    def get_actions(self, frames: Dict[int, Dict[str, Any]]) -> Dict[int, Tuple[str, torch.Tensor]]:
        from . import ops
        from .model import F32, NPATCH, Prep
        ac, dev, sl = self.actor_critic, self.device, self._slots
        if not frames:
            raise ValueError("get_actions needs the frames of at least one started slot")
        slots, ages, last = sl.rows(frames)
        obs, n, W = list(frames.values()), len(frames), self.window
        if not self._warned_window and any(a and a % W == 0 for a in ages):
            warnings.warn(f"episode longer than the {W}-step KV-cache window (max_steps): the window restarts, as the reference's step counter does")
            self._warned_window = True
        t = sl.goal_table(dev, ac.text_off)
        pos, klen = zip(*(restart_slot(a, W) for a in ages))
        hand = [int(np.asarray(o.get("an_object_is_in_hand", 0)).reshape(-1)[0]) for o in obs] if ac.has_hand else [0] * n
        # the step's one small upload, per row: cache row (= slot), ring slot to write, slots to read, age, previous action, in-hand sensor
        rows = torch.tensor([slots, pos, klen, ages, last, hand], dtype=torch.int32).to(dev)
        p = Prep()
        p.T, p.B, p.R = 1, n, n
        p.tokens = torch.empty(n, ac.ncam, NPATCH, ac.dino_dim, device=dev, dtype=ac.adt)
        for cam in range(ac.ncam):                               # only the model's cameras are read
            ops.feat_to_tokens(self._features(obs, cam).reshape(n, ac.dino_dim, NPATCH).contiguous(), p.tokens, cam, ncam=ac.ncam)
        p.time_step, p.prev_actions, p.masks = rows[3].long(), rows[4].long(), (rows[3] > 0).to(F32)
        p.hand = rows[5].long() if ac.has_hand else None
        p.traj_bt = rows[0].reshape(n, 1)                        # (one episode per row; the per-row step does not read it)
        p.ids, p.attn_mask, p.attn_mask_u8 = t.ids, t.mask, t.mask_u8
        p.U, p.L, p.S = self.num_episodes, t.L, ac.text_off + t.L
        p.ids_key = t.key                                        # eval mode: the frozen text encoder reruns only when a goal changed
        p.gid = rows[0]                                          # row -> its slot's goal
        p.row_cache, p.row_pos, p.row_klen = rows[0], rows[1], rows[2]
        if t.kvalid is not None and any(t.lens[s] < t.L for s in slots):
            p.fusion_kvalid = t.kvalid.index_select(0, rows[0].long())
        version = ac._kv_version
        ac._ensure_caches(self.num_episodes)
        if ac._kv_version != version:
            # the actor tower's caches were replaced.  Recorded acting plans are keyed by the cache version and recorded plans assert it, so none would be replayed
            # on the old caches -- but they (and the engine's recorded env-chunks, through the hooks) would keep the old caches alive and point into them: drop them
            # here, outside any recording (inside ``_ensure_caches`` the call would clear the plan table under a recording ``static_step``)
            ac.invalidate_recorded()
        logits, _, _ = ac.run_forward(p, need_grad=False)        # the actor tower (= the policy itself) alone
        _, probs, sampled, greedy = ops.policy_sample_rows(logits.view(n, -1), rows[0], rows[3], self.seed)
        picks = torch.stack([sampled, greedy]).tolist()          # the call's one host read
        names, out = self.get_action_list(), {}
        for j, s in enumerate(slots):
            sl.advance(s, picks[0][j])
            out[s] = (names[picks[1 if self.greedy_sampling else 0][j]], probs[j])
        return out
