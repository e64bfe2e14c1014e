"""Offline imitation-learning workload on the same kernels.

Mirrors ``EarlyFusionCnnTransformer`` with the llama decoder, in every ``model_version`` the reference can construct (512 x 8 and 768 x 12 on the 64-wide MFMA attention kernels; 768 x 8 = heads of 96 on the 96-wide ones, csrc/attn_hd96.hip)
(/root/reference/architecture/models/transformer_models/early_fusion_tsfm_models.py:49-207,221-312; ``VERSIONS`` below): text-conditioned multi-camera
encoder (text_cond_visual_encoder.py:56-268) -> + last-action / in-hand / time embeddings (:120-157) -> causal llama decoder ->
``actor`` -> ``nn.CrossEntropyLoss(ignore_index=-1)`` (:93,115-117); and the optimiser of ``training/offline/train_pl.py:283-287``
(AdamW, lr 1e-4).  It IS one tower of the RL model -- the RL towers are initialised from exactly these weights
(``checkpoint.init_towers_from_il``) -- so the forward/backward run the update path's kernel schedules (``model.Tower``); new here:
the batch-first IL batch format, the fused cross-entropy kernel and decoupled weight decay in the Adam kernel.

The frozen image encoder stays outside, as on the RL path: visual sensors are either pre-encoded features ``[B,T,C,7,12]`` (C = 384 DINOv2-S,
768 DINOv2-B / SigLIP-B, 1024 SigLIP-L, 2048 CLIP RN50) or uint8 frames ``[B,T,H,W,3]`` (then the frozen trunk of ``preproc`` runs first: DINOv2 and
CLIP RN50 on 224 x 384, SigLIP on 256 x 256 frames or on camera frames resized to that, preprocessors.py:35-43).  The frozen text encoder is t5-small or, for the ``siglip_*`` presets, the SigLIP text tower
(``siglip_text.SigLIPTextFrozen``: ``goals`` is then the tokenizer's id tensor [B, 64], preprocessors.py:334-343).  ``state_dict`` uses the reference's names
(``actor.weight``, no critic head), so Lightning checkpoints (``model.`` prefix) interchange.
"""
import contextlib
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import ops
from .model import BF16, CAMERAS, DINO, F32, N_ACTIONS, NPATCH, Prep, Tower, _Arena, _TowerFn, sensor_set
from .vector_slots import EpisodeSlots, goal_ids, ring_slot      # (ring_slot stays importable from here)

NAV, MANIP = CAMERAS
START_TOKEN, PAD_TOKEN = N_ACTIONS, N_ACTIONS + 1      # last_actions vocabulary (:95-101)


class _CEFn(torch.autograd.Function):
    """Fused cross-entropy forward+backward (svla_ce_loss_fwd_bwd_f32): mean over targets != ignore_index."""

    @staticmethod
    def forward(ctx, logits, target, ignore_index):
        rows, A = logits.shape
        n_valid = (target != ignore_index).sum().to(F32).reshape(1)
        dlogits = torch.empty_like(logits)
        sums = torch.zeros(1, device=logits.device, dtype=torch.float64)
        ops.ce_loss_fwd_bwd(logits.contiguous(), target.contiguous(), n_valid, dlogits, sums, ignore_index)
        ctx.save_for_backward(dlogits)
        return (sums[0] / n_valid[0].clamp(min=1.0).double()).to(F32)

    @staticmethod
    def backward(ctx, g):
        (dlogits,) = ctx.saved_tensors
        return dlogits * g, None, None


class EarlyFusionCnnTransformer(Tower):
    # model_version -> (fusion layers, decoder layers, image-feature width, text encoder); early_fusion_tsfm_models.py:221-312.  Every preset whose
    # fusion transformer and decoder are TransformerConfig(n, 512, 8), with the llama decoder (``use_llama_decoder`` defaults to True, :46):
    # DINOv2-S / -B, SigLIP-B / -L (image trunk + text tower) and CLIP RN50 (conv trunk: preproc.ClipResNet on csrc/conv.hip).
    # and the 768-wide presets whose heads are 64 wide (12 heads: siglip_base_6_3 / _6_6 / _12_12; same kernels at D = 768, llama hidden 2048).
    # TransformerConfig(n, 768, 8) = heads of 96 (base_6, and the fusion transformer of siglip_base_3_6) builds too, with its attention on the 96-wide MFMA kernels (csrc/attn_hd96.hip).
    # Four more names cannot be constructed in the reference as shipped: small_3_nonTxEnc / siglip_base_3_nonTxEnc (``globals()["NonTxMultiCameraVisualEncoder"]``, :64, is a KeyError: the class is not
    # imported into that module, :22-28) and siglip_base_384_3 / siglip_base_384_resize_3 (image encoders absent from IMAGE_ENCODERS, image_encoders.py:103-112).
    VERSIONS = {"small": (3, 3, 384, "t5-small"), "small_3": (3, 3, 384, "t5-small"), "small_6": (6, 6, 384, "t5-small"), "base_3": (3, 3, 768, "t5-small"),
                "siglip_base_3": (3, 3, 768, "SigLIPBase"), "siglip_3": (3, 3, 768, "SigLIPBase"), "siglip_base_3_llama": (3, 3, 768, "SigLIPBase"),
                "siglip_base_6": (6, 6, 768, "SigLIPBase"), "siglip_large_3": (3, 3, 1024, "SigLIPLarge"), "clip_resnet_50_3": (3, 3, 2048, "t5-small"),
                "siglip_base_6_3": (6, 3, 768, "SigLIPBase", 768, 12), "siglip_base_6_6": (6, 6, 768, "SigLIPBase", 768, 12),
                "siglip_base_12_12": (12, 12, 768, "SigLIPBase", 768, 12),
                # heads of 96 (768 / 8): attention on the 96-wide MFMA kernels (ops.attn_fwd head_dim = 96; SVLA_ATTN96_F32=1: the fp32 detour), everything else as above
                "base_6": (6, 6, 768, "t5-small", 768, 8), "siglip_base_3_6": (3, 6, 768, "SigLIPBase", 768, 8, 12)}

    def __init__(self, device="cuda", max_length: int = 1000, input_sensors=(NAV, MANIP, "last_actions", "an_object_is_in_hand"),
                 image_preprocessor=None, n_fusion_layers: int = 3, n_decoder_layers: int = 3, dino_dim: int = DINO, text_encoder: str = "t5-small", d_model: int = 512, n_heads: int = 8,
                 n_heads_decoder: Optional[int] = None, data_augmentation: bool = False, skip_padded_steps: bool = False):
        if not torch.cuda.is_available():
            raise RuntimeError("safevla_amd needs an MI355X: there is no CPU or eager fallback for the policy kernels")
        ops.lib()
        arena = _Arena()
        device = torch.device(device)
        # ``input_sensors`` decides what is built, as in the reference (early_fusion_tsfm_models.py:90-102, text_cond_visual_encoder.py:101-111): a camera token per
        # listed camera, ``last_actions_embed`` only with "last_actions", ``object_in_hand_embed`` only with "an_object_is_in_hand"; unknown names are a ValueError
        cameras, in_hand, prev_actions = sensor_set(input_sensors)
        super().__init__(arena, device, n_fusion_layers=n_fusion_layers, n_decoder_layers=n_decoder_layers, max_steps=max_length, dino_dim=dino_dim,
                         text_encoder=text_encoder, d_model=d_model, n_heads=n_heads, n_heads_decoder=n_heads_decoder, cameras=cameras, in_hand=in_hand,
                         prev_actions=prev_actions)
        arena.build(device)
        self.bind()
        self.towers = [self]
        self.input_sensors = list(input_sensors)
        self.image_preprocessor = image_preprocessor
        # data_augmentation (train_pl.py:92, early_fusion_tsfm_models.py:342-343: the random v2 list, preprocessors.py:86-118): forward(batch) passes each camera's
        # uint8 frames [B,T,H,W,3] through that camera's augmenter -- one newly drawn transform per trajectory -- in front of the frozen trunk; the SigLIP presets
        # augment at their 256 x 256 input size, behind the resize.  Seed a camera's draws through ``augmenters[cam].generator``.  Pre-encoded features pass untouched.
        self.data_augmentation = bool(data_augmentation)
        if self.data_augmentation:
            from .preproc import RandomDataAugmenter
            size = (256, 256) if text_encoder.startswith("SigLIP") else None
            self.augmenters = [RandomDataAugmenter(size=size) for _ in self.cameras]
        # skip_padded_steps: a batch that holds ``lengths`` (int [B], the valid steps of each trajectory: ``Preprocessor.process`` below, preprocessors.py:294-296) runs
        # everything in front of the decoder on the valid steps only (``prepare``).  Off, or without ``lengths``, or with every length equal to T: today's path.
        self.skip_padded_steps = bool(skip_padded_steps)
        self._anchor = torch.zeros(1, device=device, requires_grad=True)
        self.sync_weights()

    # ---- weights: reference names ------------------------------------------------------------------------------------------
    @staticmethod
    def _to_ref(k: str) -> Optional[str]:
        if k.startswith("critic."):
            return None
        return k.replace("actor.linear.", "actor.")

    def state_dict(self, *a, **kw):
        sd = super().state_dict(*a, **kw)
        return type(sd)((self._to_ref(k), v) for k, v in sd.items() if self._to_ref(k) is not None)

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        own = super().state_dict()
        sd = {k.replace("actor.weight", "actor.linear.weight").replace("actor.bias", "actor.linear.bias"): v for k, v in state_dict.items()}
        missing = [k for k in own if k not in sd and not k.startswith("critic.")]
        unexpected = [k for k in sd if k not in own and "visual_encoder.image_encoder" not in k]
        if strict and (missing or unexpected):
            raise RuntimeError(f"state_dict mismatch: missing {missing[:5]}, unexpected {unexpected[:5]}")
        with torch.no_grad():
            for k, v in sd.items():
                if k in own:
                    own[k].copy_(v.to(own[k].device, own[k].dtype))
        self.sync_weights()
        return missing, unexpected

    def sync_weights(self):
        ar = self.arena
        ops.cast_bf16(ar.flat_p, ar.flat_bf16)
        self.refresh_transposes()
        self.visual_encoder.text_encoder.sync()
        self._t5_cache = (None, None)

    def zero_grad(self, set_to_none: bool = False):
        self.arena.flat_g.zero_()

    def trainable_parameters(self):
        return [p for n, p in self.named_parameters() if p.requires_grad and not n.startswith("critic.")]

    # ---- batch -> kernel inputs ----------------------------------------------------------------------------------------------
    @torch.no_grad()
    def prepare(self, batch: Dict, augment: bool = False) -> Prep:
        dev = self.device_
        B, T = batch[self.cameras[0]].shape[:2]
        R = T * B
        rag = self._compact_rows(batch, B, T)                    # None: every step of the [B, T] batch runs (checked and built on the host, before the first launch)
        p = Prep()
        p.T, p.B, p.R = T, B, R
        p.acting = False                                         # forward(batch): whole windows, also when T = 1 (the agent's single steps set it)
        Rf = R
        if rag is not None:
            # one upload per batch: decoder row -> compact row | compact row -> decoder row | compact row -> row (b * T + t) of the batch | goal of a compact row |
            # first compact row of every goal
            Rf = rag["Rf"]
            tab = torch.from_numpy(rag["table"]).to(dev)
            p.Rf, p.row_map, p.row_inv, row_src, gid_c, p.row_seg = (Rf,) + tuple(torch.split(tab, [R, Rf, Rf, Rf, B + 1]))
        p.tokens = torch.empty(Rf, self.ncam, NPATCH, self.dino_dim, device=dev, dtype=BF16)
        for cam, key in enumerate(self.cameras):                 # only the model's sensors are read from the batch
            x = batch[key].to(dev)
            if x.dtype == torch.uint8:                           # raw frames [B,T,H,W,3] -> frozen ViT
                if self.image_preprocessor is None:
                    self.image_preprocessor = self._frozen_image_encoder(key, dev)
                if augment:
                    x = self.augmenters[cam].augment_u8(x)       # (one transform per trajectory, drawn as without the skip: padded frames are augmented, then left behind)
                if rag is not None:                              # the valid frames only, trajectory by trajectory, straight out of the [B * T] batch
                    x, nb = x.contiguous(), x[0, 0].numel()
                    fr = torch.empty(Rf, *x.shape[2:], device=dev, dtype=torch.uint8)
                    ops.rows_gather(fr, nb, x, nb, row_src, Rf, nb, R)
                else:
                    fr = x.transpose(0, 1).reshape(R, *x.shape[2:]).contiguous()
                self.image_preprocessor.process_tokens(fr, p.tokens, cam, ncam=self.ncam)
            elif rag is not None:                                # pre-encoded features: the valid steps' [C, 84] fp32 rows; a padded step's are never read
                x, nb = x.float().contiguous(), self.dino_dim * NPATCH * 4
                ft = torch.empty(Rf, self.dino_dim, NPATCH, device=dev, dtype=F32)
                ops.rows_gather(ft, nb, x, nb, row_src, Rf, nb, R)
                ops.feat_to_tokens(ft, p.tokens, cam, ncam=self.ncam)
            else:                                                # pre-encoded features [B,T,384,7,12]
                ops.feat_to_tokens(x.transpose(0, 1).reshape(R, self.dino_dim, NPATCH).contiguous().float(), p.tokens, cam, ncam=self.ncam)
        tb = lambda v: v.to(dev).transpose(0, 1).reshape(R).contiguous()     # [B,T] -> rows (t*B + b)
        p.prev_actions = p.masks = p.hand = None
        if self.has_prev:
            la = tb(batch["last_actions"]).to(torch.int64)
            p.prev_actions = la
            p.masks = (la != START_TOKEN).to(F32)                # start token <=> "no previous action" (mask 0 selects row 20)
        if self.has_hand:
            p.hand = tb(batch["an_object_is_in_hand"]).to(torch.int64) if "an_object_is_in_hand" in batch else torch.zeros(R, device=dev, dtype=torch.int64)
        p.time_step = tb(batch["time_ids"]).to(torch.int64)
        p.traj_bt = torch.arange(B, device=dev, dtype=torch.int32)[:, None].expand(B, T).contiguous()   # one trajectory per row: causal
        goals = batch["goals"]
        if self.text_encoder_name == "t5-small":                 # HF tokenizer output (preprocessors.py:157-163)
            p.ids = goals["input_ids"].to(dev).to(torch.int64).contiguous()
            p.attn_mask = goals["attention_mask"].to(dev).to(torch.int64).contiguous()
            p.U, p.L = p.ids.shape
        else:                                                    # open_clip tokenizer output: ids [B, context] (preprocessors.py:334-343); + the pooled token
            p.ids = (goals["input_ids"] if isinstance(goals, dict) else goals).to(dev).to(torch.int64).contiguous()
            p.attn_mask = torch.ones_like(p.ids)
            p.U, p.L = p.ids.shape[0], self.visual_encoder.text_encoder.out_tokens(p.ids.shape[1])
        p.gid = (torch.arange(R, device=dev) % B).to(torch.int32).contiguous() if rag is None else gid_c
        p.S = self.text_off + p.L
        return p

    def _compact_rows(self, batch: Dict, B: int, T: int):
        """The host half of ``skip_padded_steps``: None when the batch runs as it always has (flag off, no ``lengths``, or every length equal to T); else the compact row
        numbering -- the valid steps, trajectory by trajectory, so that one goal's rows are contiguous -- as one int32 table (``prepare`` names its parts).  Reads
        ``lengths`` (the one host read the skip needs; none if it is a host tensor) and launches nothing; what cannot run is a ValueError here."""
        if not self.skip_padded_steps or batch.get("lengths") is None:
            return None
        lens = np.asarray(torch.as_tensor(batch["lengths"]).reshape(-1).tolist(), dtype=np.int64)
        if lens.shape[0] != B:
            raise ValueError(f"lengths holds {lens.shape[0]} entries for a batch of {B} trajectories")
        if lens.min() < 1 or lens.max() > T:
            raise ValueError(f"lengths {lens.tolist()}: every trajectory has 1 ... {T} valid steps (T = the padded window)")
        if (lens == T).all():
            return None
        goals = batch["goals"]
        n_goals = int((goals["input_ids"] if isinstance(goals, dict) else goals).shape[0])
        if n_goals != B:
            raise ValueError(f"skip_padded_steps: {n_goals} goals for {B} trajectories (one goal per trajectory: a goal's compact rows are one segment)")
        if self.fp8_attention or self.adt != BF16 or self._frame_rows_unaligned(batch):
            raise ValueError("skip_padded_steps is not carried through fp8_attention, the fp32 verification mode, or uint8 frames whose H * W * 3 is not a multiple of "
                             f"16 bytes (fp8_attention = {self.fp8_attention}, dtype = {self.adt}): build the model without the flag, or leave ``lengths`` out")
        R, seg = T * B, np.concatenate([[0], np.cumsum(lens)])
        Rf = int(seg[-1])
        b_of = np.repeat(np.arange(B), lens)
        t_of = np.arange(Rf) - seg[b_of]
        inv = t_of * B + b_of                                    # compact row -> decoder row (t * B + b)
        fwd = np.full(R, -1, dtype=np.int64)
        fwd[inv] = np.arange(Rf)
        return dict(Rf=Rf, table=np.concatenate([fwd, inv, b_of * T + t_of, b_of, seg]).astype(np.int32))

    def _frame_rows_unaligned(self, batch: Dict) -> bool:
        """a camera's uint8 frames whose bytes per frame the 16-byte row gather cannot take (the presets' 224 x 384 and 256 x 256 frames can)"""
        return any(batch[k].dtype == torch.uint8 and batch[k][0, 0].numel() % 16 for k in self.cameras)

    def _frozen_image_encoder(self, key, dev):
        """IMAGE_ENCODERS of image_encoders.py:103-112 for raw uint8 frames, by preset: DINOv2 (224 x 384), the SigLIP trunk (256 x 256; other sizes are resized) or,
        for clip_resnet_50_3 (2048-wide features), the CLIP RN50 conv trunk (224 x 384)."""
        from .preproc import ClipResNetPreprocessor, DinoViTPreprocessor, SigLIPDataAugmentationPreprocessor, SigLIPPreprocessor
        if self.text_encoder_name.startswith("SigLIP"):
            # SigLipPreprocessor of preprocessors.py:319-328: tensor_image_preprocessor(size=(256, 256)) resizes camera-sized frames in front of the trunk (one
            # resizing front per camera; 256 x 256 frames pass through it untouched)
            resize = [SigLIPDataAugmentationPreprocessor(k, k, device=dev) for k in self.cameras]
            return SigLIPPreprocessor(key, key, siglip_model_type={768: "ViT-B-16-SigLIP-256", 1024: "ViT-L-16-SigLIP-256"}[self.dino_dim], device=dev, augmenter=resize)
        if self.dino_dim == 2048:
            return ClipResNetPreprocessor(key, key, device=dev)
        return DinoViTPreprocessor(key, key, dino_model_type={384: "dinov2_vits14", 768: "dinov2_vitb14", 1024: "dinov2_vitl14"}[self.dino_dim], device=dev)

    # ---- reference forward API --------------------------------------------------------------------------------------------------
    def _logits_tb(self, batch: Dict) -> torch.Tensor:
        """the logits of ``_forward_tb`` alone"""
        return self._forward_tb(batch)[0]

    def _targets_tb(self, batch: Dict, prep: Prep) -> torch.Tensor:
        """``batch["actions"]`` as int64 rows (t * B + b).  With padded steps skipped, a padded step's target is the ignore index whatever the batch holds there (set on
        the device from the row table): its logits come from a zero fusion feature and mean nothing."""
        tgt = batch["actions"].to(self.device_).transpose(0, 1).reshape(-1).to(torch.int64)
        return tgt if prep.row_map is None else torch.where(prep.row_map >= 0, tgt, torch.full_like(tgt, -1))

    def _forward_tb(self, batch: Dict):
        """The tower forward of a batch -> (logits [T, B, A] fp32, rows in the kernels' order (t * B + b); its Prep); shared by forward(batch) and ILTrainer.validation_step"""
        # whole episodes (512 < T <= 1000 steps) run forward only -- under torch.no_grad() or in eval mode; what cannot run is refused before the first launch
        self._check_seq_len(int(batch[self.cameras[0]].shape[1]), torch.is_grad_enabled() and self.training)
        prep = self.prepare(batch, augment=self.data_augmentation)
        logits, _, _ = _TowerFn.apply(self._anchor, self, prep, True, False)      # [T, B, A] fp32
        return logits, prep

    def forward(self, batch: Dict) -> Dict[str, torch.Tensor]:
        logits, prep = self._forward_tb(batch)
        out = dict(actions_logits=logits.transpose(0, 1))
        if "actions" in batch:
            tgt = self._targets_tb(batch, prep)
            loss = _CEFn.apply(logits.reshape(-1, N_ACTIONS), tgt, -1)
            out["actions_loss"] = loss
            out["loss"] = loss
        return out

    @classmethod
    def build_agent(cls, model_version="small_3", input_sensors=(NAV, MANIP, "last_actions", "an_object_is_in_hand"), loss="action", device="cuda",
                    sampling="greedy", data_augmentation: bool = False, ckpt_pth: Optional[str] = None, skip_padded_steps: bool = False, **kw):
        """``build_agent`` of early_fusion_tsfm_models.py:352-363: the model of ``build_model`` wrapped in its online agent.  ``data_augmentation`` reaches the
        model's forward(batch) only: the agent's single steps act on the frames as they come."""
        return EarlyFusionCnnTransformerAgent(cls.build_model(model_version, input_sensors, loss, data_augmentation, device=device, ckpt_pth=ckpt_pth,
                                                              skip_padded_steps=skip_padded_steps), device, sampling, **kw)

    @classmethod
    def build_vector_agent(cls, model_version="small_3", input_sensors=(NAV, MANIP, "last_actions", "an_object_is_in_hand"), loss="action", device="cuda",
                           sampling="greedy", num_episodes: int = 1, max_seq_len: int = 1000, tokenizer=None, generator: Optional[torch.Generator] = None,
                           ckpt_pth: Optional[str] = None, skip_padded_steps: bool = False):
        """The model of ``build_model`` behind ``EarlyFusionCnnTransformerVectorAgent``: ``num_episodes`` evaluation episodes served by one set of weights."""
        return EarlyFusionCnnTransformerVectorAgent(cls.build_model(model_version, input_sensors, loss, device=device, ckpt_pth=ckpt_pth,
                                                                    skip_padded_steps=skip_padded_steps), num_episodes, device, sampling, max_seq_len=max_seq_len, tokenizer=tokenizer, generator=generator)

    @classmethod
    def version_config(cls, model_version):
        """(fusion layers, decoder layers, image-feature width, text encoder, transformer width, fusion heads, decoder heads) of a preset"""
        v = cls.VERSIONS[model_version]
        v = v + (512, 8)[len(v) - 4:] if len(v) < 6 else v
        return v if len(v) == 7 else v + (v[5],)

    @classmethod
    def build_model(cls, model_version="small_3", input_sensors=(NAV, MANIP, "last_actions", "an_object_is_in_hand"), loss="action",
                    data_augmentation: bool = False, device="cuda", ckpt_pth: Optional[str] = None, ckpt_prefix: str = "model.", skip_padded_steps: bool = False):
        if model_version not in cls.VERSIONS:
            raise NotImplementedError(f"model_version {model_version!r}: built are {sorted(cls.VERSIONS)} (512-wide fusion transformer + llama decoder; "
                                      "early_fusion_tsfm_models.py:221-312)")
        nf, nd, dd, te, dm, nh, nhd = cls.version_config(model_version)
        m = cls(device=device, input_sensors=input_sensors, n_fusion_layers=nf, n_decoder_layers=nd, dino_dim=dd, text_encoder=te, d_model=dm, n_heads=nh,
                n_heads_decoder=nhd, data_augmentation=data_augmentation, skip_padded_steps=skip_padded_steps)
        if ckpt_pth is not None:    # Lightning checkpoint (training/offline/train_utils.py:6-68)
            sd = torch.load(ckpt_pth, map_location="cpu")["state_dict"]
            m.load_state_dict({k[len(ckpt_prefix):]: v for k, v in sd.items() if k.startswith(ckpt_prefix)}, strict=False)
        return m


def _default_action_list():
    from .agent import ALL_STRETCH_ACTIONS
    return list(ALL_STRETCH_ACTIONS)


@dataclass
class PreprocessorConfig:
    """``PreprocessorConfig`` of preprocessors.py:63-73, for the fields that decide a batch here: ``max_steps`` (truncation), ``action_list``, ``goal_sensor_uuid``;
    plus ``input_sensors`` (what the model was built for: ``model.input_sensors``) and ``text_encoder`` (the preset's, ``EarlyFusionCnnTransformer.version_config``).
    The reference always pads (``pad = True`` is its only trained setting) and resizes / normalises the frames in this class (``image_size``, ``data_augmentation``):
    here frames stay uint8 at the camera's size and both live in front of the frozen trunk (``EarlyFusionCnnTransformer(data_augmentation=...)``, preproc.py)."""
    input_sensors: Sequence[str] = (NAV, MANIP, "last_actions", "an_object_is_in_hand")
    max_steps: Optional[int] = None
    action_list: List[str] = field(default_factory=_default_action_list)
    goal_sensor_uuid: str = "goals"
    text_encoder: str = "t5-small"
    text_encoder_context_length: int = 64


class Preprocessor:
    """``Preprocessor.process`` of preprocessors.py:246-303 (the step in front of the model in ``LitModel.forward_batch``, train_pl.py:144-152): a list of samples
    ``{"observations": {...}}`` of unequal length, as the dataset yields them, -> one padded batch for ``EarlyFusionCnnTransformer.forward`` / ``ILTrainer``.

    Per key of the first sample's observations, in its order (:252-285):
      a camera of ``input_sensors``   uint8 [t, H, W, 3] per sample -> uint8 [B, Tmax, H, W, 3], zero frames behind a trajectory's end (pad_sequence with 0, :101-107; the
                                      reference pads the normalised float frames, here the frames stay uint8 and the trunk's front normalises them);
      "actions"                       action strings -> int64 indices into ``action_list``, padding -1 (:120-136); an unknown string is a KeyError, as there;
      "last_actions"                  the same vocabulary plus "" -> len(action_list) = 20, the start token (:80-83); padding len(action2idx) = 21 (:138-156);
      "an_object_is_in_hand"          int64, padding 2 (:206-216);         "time_ids"    int64, padding -1 (:195-204);
      "goal"                          -> ``cfg.goal_sensor_uuid``: strings through the tokenizer (t5 presets: ``tokenizer(goals, return_tensors="pt", padding=True)`` -> a dict
                                      of input_ids / attention_mask, :158-164; SigLIP presets: ``tokenizer(goals, context_length=...)`` -> an id tensor, :334-343); goals
                                      that are already tokenised (a dict of 1-D ids and mask, or a 1-D id tensor, per sample) pass through: right-padded with id 0 /
                                      mask 0 to the longest (t5) or stacked (SigLIP);
      "initial_agent_location", "templated_task_type"      ignored (:284);
    and ``lengths`` int32 [B] with ``padding_mask`` bool [B, Tmax], True = padded (:241-244, 287-301).  Every per-step key is cut to ``max_steps`` first (:111,130,150,197,208).
    The reference reports the UNCUT length of "actions" in ``lengths`` (:294-296); here it is the length after the cut, min(len, max_steps), so that ``lengths`` describes
    the tensors next to it -- ``padding_mask`` is the same either way.  Without "actions" the length is read from the first camera (the reference picks a random one, :290-292).

    The keys follow the model: a camera, "last_actions" or "an_object_is_in_hand" that ``input_sensors`` does not list, or any key the reference's ``process`` knows
    (visibility, rooms_seen, the bbox sensors, relative_arm_location_metadata, ...) or does not know, is a ValueError that names it (the reference: NotImplementedError
    for the unknown, :283-285).  Works on ``device="cpu"``."""

    _ALWAYS, _IGNORED = ("actions", "goal", "time_ids"), ("initial_agent_location", "templated_task_type")

    def __init__(self, cfg: Optional[PreprocessorConfig] = None, device="cuda", tokenizer=None):
        self.cfg = cfg = cfg if cfg is not None else PreprocessorConfig()
        self.device = torch.device(device)
        self.cameras, self.has_hand, self.has_prev = sensor_set(cfg.input_sensors)
        self.action2idx = {a: i for i, a in enumerate(cfg.action_list)}
        self.action2idx[""] = len(cfg.action_list)               # start-of-sequence token of last_actions (:81-83)
        if tokenizer is None and cfg.text_encoder == "t5-small":
            from .text import GoalTokenizer
            tokenizer = GoalTokenizer()
        self.tokenizer = tokenizer

    @property
    def num_actions(self):
        return len(self.action2idx)

    def _pad(self, rows, value):
        return torch.nn.utils.rnn.pad_sequence(rows, batch_first=True, padding_value=value).to(self.device)

    def _steps(self, batch, key, value, dtype=torch.int64):
        return self._pad([torch.as_tensor(np.asarray(s[key][:self.cfg.max_steps])).to(dtype).reshape(-1) for s in batch], value)

    def _words(self, batch, key, value):
        return self._pad([torch.tensor([self.action2idx[a] for a in s[key][:self.cfg.max_steps]], dtype=torch.int64) for s in batch], value)

    def _frames(self, batch, key):
        frames = [torch.as_tensor(s[key][:self.cfg.max_steps]) for s in batch]
        if any(f.dtype != torch.uint8 or f.dim() != 4 or f.shape[-1] != 3 for f in frames):
            raise ValueError(f"{key}: uint8 frames [t, H, W, 3] per sample, got {[(str(f.dtype), tuple(f.shape)) for f in frames][:3]}")
        return self._pad(frames, 0)

    def _goals(self, batch):
        goals = [s["goal"] for s in batch]
        t5 = self.cfg.text_encoder == "t5-small"
        if all(isinstance(g, str) for g in goals):
            if self.tokenizer is None:
                raise ValueError("string goals need a tokenizer (SigLIP presets: open_clip's tokenizer is not available offline; pass tokenised goals or tokenizer=)")
            if t5:
                return {k: v.to(self.device) for k, v in self.tokenizer(goals, return_tensors="pt", padding=True).items()}
            return torch.as_tensor(self.tokenizer(goals, context_length=self.cfg.text_encoder_context_length)).to(self.device)
        if any(isinstance(g, str) for g in goals):
            raise ValueError("goals: strings and tokenised goals in one batch")
        one = lambda v: torch.as_tensor(np.asarray(v)).to(torch.int64).reshape(-1)
        if all(isinstance(g, dict) for g in goals):
            return {k: self._pad([one(g[k]) for g in goals], 0) for k in ("input_ids", "attention_mask")}
        ids = [one(g) for g in goals]
        if t5:                                                       # bare ids for a t5 preset: the mask is where they are
            return dict(input_ids=self._pad(ids, 0), attention_mask=self._pad([torch.ones_like(i) for i in ids], 0))
        return torch.stack(ids).to(self.device)

    def process(self, batch):
        if len(batch) == 0:
            return None
        batch = [s["observations"] for s in batch]
        keys, out = list(batch[0].keys()), dict()
        for key in keys:
            if key in self.cameras:
                out[key] = self._frames(batch, key)
            elif key == "an_object_is_in_hand" and self.has_hand:
                out[key] = self._steps(batch, key, 2)
            elif key == "last_actions" and self.has_prev:
                out[key] = self._words(batch, key, len(self.action2idx))
            elif key == "actions":
                out[key] = self._words(batch, key, -1)
            elif key == "time_ids":
                out[key] = self._steps(batch, key, -1)
            elif key == "goal":
                out[self.cfg.goal_sensor_uuid] = self._goals(batch)
            elif key not in self._IGNORED:
                raise ValueError(f"sensor {key!r}: the model is built for {list(self.cfg.input_sensors)} (+ {list(self._ALWAYS)}; ignored: {list(self._IGNORED)})")
        look = "actions" if "actions" in keys else next((k for k in keys if k in self.cameras), None)
        if look is None:
            raise ValueError(f"samples hold neither 'actions' nor a camera of {list(self.cameras)}: no length to read")
        cut = self.cfg.max_steps
        out["lengths"] = torch.tensor([len(s[look]) if cut is None else min(len(s[look]), cut) for s in batch], dtype=torch.int32).to(self.device)
        out["padding_mask"] = torch.arange(out[look].shape[1], device=self.device)[None, :] >= out["lengths"][:, None]
        return out


def f1_from_counts(C) -> Dict:
    """Per-class, macro and weighted F1 of a confusion matrix C[target, pred] (numpy or CPU torch, any integer dtype) -> dict(f1 = list of A, f1_macro, f1_weighted).

    [3P] RESTATED, UNPINNED: this is how torchmetrics' multiclass ``F1Score`` (``average`` = None / "macro" / "weighted", top_k = 1, zero_division = 0; the three
    objects of train_pl.py:200-207) reads, restated from its documentation -- torchmetrics is neither in the reference tree nor available offline, so nothing here
    is compared against it.  With tp_k = C[k, k], fp_k = column sum - tp_k, fn_k = row sum - tp_k:
      f1_k     = 2 tp_k / (2 tp_k + fp_k + fn_k), 0 where that denominator is 0;
      macro    = mean of f1_k over the classes with tp_k + fp_k + fn_k > 0 (a class in neither targets nor predictions does not count);
      weighted = sum_k (tp_k + fn_k) f1_k / sum_k (tp_k + fn_k)  (weights = the classes' support);
    both 0.0, never NaN, when no class qualifies.  Rows with the ignored target never reach C.  Equal to sklearn.metrics.f1_score(labels=None) for the three averages
    (tests/test_il_f1_cpu.py, where sklearn is installed)."""
    C = np.asarray(C).astype(np.float64)
    if C.ndim != 2 or C.shape[0] != C.shape[1]:
        raise ValueError(f"f1_from_counts: a square confusion matrix, got {C.shape}")
    tp = np.diag(C)
    fp, fn = C.sum(0) - tp, C.sum(1) - tp
    den = 2.0 * tp + fp + fn
    f1 = np.divide(2.0 * tp, den, out=np.zeros_like(den), where=den > 0)
    seen, support = den > 0, tp + fn
    macro = float(f1[seen].mean()) if seen.any() else 0.0
    weighted = float((support * f1).sum() / support.sum()) if support.sum() > 0 else 0.0
    return dict(f1=[float(v) for v in f1], f1_macro=macro, f1_weighted=weighted)


class ActionF1:
    """The validation state of one epoch: the confusion matrix (target, greedy action) and the summed cross-entropy of every batch seen, kept where the logits are.
    ``update`` is one launch of svla_action_metrics_f32 (csrc/metrics.hip) -- no host read, no allocation; ``reduce_`` sums the state over the ranks; ``compute`` is
    the epoch's one host read.  The state is one int64 buffer: ``counts`` [A, A] views its first A * A words, ``sums`` [3] (loss sum, frames, refused rows) views the
    last three as fp64.  On ``device="cpu"`` everything but ``update`` works (the reduction and the arithmetic are tested without a GPU)."""

    def __init__(self, num_actions: int = N_ACTIONS, ignore_index: int = -1, device="cuda"):
        if not 1 <= num_actions <= 64:
            raise ValueError(f"num_actions = {num_actions}: svla_action_metrics_f32 takes 1 ... 64 actions")
        self.num_actions, self.ignore_index = num_actions, ignore_index
        self.state = torch.zeros(num_actions * num_actions + 3, device=device, dtype=torch.int64)
        self.counts = self.state[:num_actions * num_actions].view(num_actions, num_actions)
        self.sums = self.state[num_actions * num_actions:].view(torch.float64)

    def update(self, logits_rows: torch.Tensor, target_rows: torch.Tensor):
        """logits_rows [rows, A] fp32 (dense rows, any row stride), target_rows [rows] int64"""
        ops.action_metrics(logits_rows, target_rows, self.counts, self.sums, self.ignore_index)

    def reduce_(self):
        """Every rank leaves with the sum of all ranks' states (a no-op on a single process)"""
        from . import parallel
        parallel.allreduce_sum_(self.counts)
        parallel.allreduce_sum_(self.sums)

    def compute(self) -> Dict:
        """-> dict(f1, f1_macro, f1_weighted, loss, frames, confusion).  Raises if any row was refused: a diverged model (NaN logits) or a target outside
        [0, A) must not report an F1."""
        A = self.num_actions
        host = self.state.cpu()                                  # the epoch's one host read
        C, sums = host[:A * A].view(A, A).numpy(), host[A * A:].view(torch.float64).tolist()
        if sums[2] > 0:
            raise ValueError(f"validation refused {int(sums[2])} rows (NaN logits or a target outside [0, {A}) that is not ignore_index = {self.ignore_index}): no F1")
        out = f1_from_counts(C)
        out.update(loss=sums[0] / max(sums[1], 1.0), frames=int(sums[1]), confusion=C.copy())
        return out

    def reset(self):
        self.state.zero_()


@contextlib.contextmanager
def deterministic_gradients(model: EarlyFusionCnnTransformer, n_rows: int):
    """Inside, the backward of ``model`` accumulates its gradients across workgroups as 64-bit fixed-point integers in a shadow of the flat gradient buffer
    (svla_det_config: integer addition is associative, so two passes over the same inputs leave the same bits); on leaving, the shadow is folded into
    ``model.arena.flat_g`` and unregistered.  ``n_rows``: the steps of the batch, which sets the shadow's grid as the RL engine does (``ops.det_grid_bits``: the
    partial sums of a mean over fewer rows are larger).  ``ops.det_bypass_count()`` afterwards tells how many partials were too large for the shadow (0: repeatable)."""
    g = model.arena.flat_g
    shadow = getattr(model, "_det_shadow", None)
    if shadow is None or shadow.numel() != g.numel():
        shadow = model._det_shadow = torch.zeros(g.numel(), device=g.device, dtype=torch.int64)
    ops.det_set_grid(ops.det_grid_bits(n_rows))
    ops.det_config(0, g, shadow)
    try:
        yield
    finally:
        ops.det_finalize(g, shadow)
        ops.det_config(0, None, None)


class ILTrainer:
    """``LitModel.training_step`` + ``configure_optimizers`` (training/offline/train_pl.py:154-186,283-287): AdamW(lr) on the flat arena; and its
    ``validation_step`` / ``on_validation_epoch_end`` (:187-281) on the F1 state of ``ActionF1``."""

    def __init__(self, model: EarlyFusionCnnTransformer, lr: float = 1e-4, weight_decay: float = 0.01, betas=(0.9, 0.999), eps: float = 1e-8,
                 deterministic: bool = False):
        self.model, self.lr, self.wd, self.betas, self.eps = model, lr, weight_decay, betas, eps
        self.step_count = 0
        # deterministic: bitwise-repeatable gradients -- every cross-workgroup accumulation of the backward in 64-bit fixed point (``deterministic_gradients``), as
        # PPOLagConfig(deterministic=True) does for the RL update
        self.deterministic = bool(deterministic)
        self.val_metrics = ActionF1(N_ACTIONS, -1, device=model.device_)

    def validation_step(self, batch: Dict) -> None:
        """One held-out batch into the epoch's metrics (train_pl.py:187-207): the tower forward of ``forward(batch)`` in eval mode under ``torch.no_grad()`` (so windows of
        513 ... 1024 steps validate), then ONE launch on the [T * B, A] logits: argmax, confusion counts and the summed cross-entropy (padded steps, actions = -1, add
        nothing).  svla_ce_loss_fwd_bwd_f32 does not run; nothing is returned and nothing is read back.  The train / eval mode of the model is put back."""
        m = self.model
        was_training = m.training
        m.eval()
        try:
            with torch.no_grad():
                logits, prep = m._forward_tb(batch)
                tgt = m._targets_tb(batch, prep)                      # rows (t * B + b), as forward(batch) orders them
                self.val_metrics.update(logits.reshape(-1, N_ACTIONS), tgt)
        finally:
            m.train(was_training)

    def validation_epoch_end(self) -> Dict[str, float]:
        """The reference's log keys of a validation epoch (train_pl.py:252-281): f1score_weighted/val, f1score_macro/val, f1score/<action>/val for the 20 names of
        ALL_STRETCH_ACTIONS, actions_loss/val and loss/val, plus val_frames (the non-padded steps seen, over all ranks).  Lightning logs the loss per step and averages
        the steps' means; this is the epoch's mean over the valid steps instead.  Sums the state over the ranks, reads it once, and starts the next epoch at zero."""
        from .agent import ALL_STRETCH_ACTIONS
        vm = self.val_metrics
        vm.reduce_()
        try:
            r = vm.compute()
        finally:
            vm.reset()
        out = {"f1score_weighted/val": r["f1_weighted"], "f1score_macro/val": r["f1_macro"]}
        out.update({f"f1score/{name}/val": v for name, v in zip(ALL_STRETCH_ACTIONS, r["f1"])})
        out.update({"actions_loss/val": r["loss"], "loss/val": r["loss"], "val_frames": r["frames"]})
        return out

    def training_step(self, batch: Dict) -> Dict[str, float]:
        m = self.model
        m.zero_grad()
        if self.deterministic:
            B, T = batch[m.cameras[0]].shape[:2]
            with deterministic_gradients(m, B * T):
                out = m(batch)
                out["loss"].backward()
        else:
            out = m(batch)
            out["loss"].backward()
        self.step_count += 1
        ar = m.arena
        ops.adam_step(ar.flat_p, ar.flat_g, ar.flat_m, ar.flat_v, ar.flat_bf16, self.lr, self.step_count, self.betas[0], self.betas[1],
                      self.eps, weight_decay=self.wd)
        m.refresh_transposes()
        return {"loss": float(out["loss"].detach())}

    def state_dict(self):
        ar = self.model.arena
        return dict(step=self.step_count, exp_avg=ar.flat_m.clone(), exp_avg_sq=ar.flat_v.clone())


class EarlyFusionCnnTransformerAgent:
    """Online agent of the imitation-learning model: ``EarlyFusionCnnTransformerAgent`` of early_fusion_tsfm_models.py:366-520 behind ``AbstractAgent``
    (architecture/agent.py:5-51) -- ``reset()``, ``get_action_list()``, ``get_action(observations, goal_spec) -> (action_str, action_probs)``.

    One call = the step's sensors (uint8 frames -> the preset's frozen image trunk, or pre-encoded features) + the cached goal -> a single-step forward of the tower
    against the llama KV caches (the acting path of ``model.Tower``: the reference re-embeds the step, appends it to ``cache["embedded_features"]`` and calls the
    decoder with ``start_pos = curr_t``, :476-499 -- the same per-step arithmetic) -> greedy or sampled action; the previous action fed to the next step is the
    chosen action index (:512-513), the first step's is the start token (:416-420).

    ``goal_spec``: a string (tokenised by ``tokenizer``: for the t5 presets ``text.GoalTokenizer`` -- the real ``t5-small`` vocabulary through its ``spiece_model`` --,
    for the SigLIP presets any callable ``tokenizer([text], context_length=64) -> ids [1, 64]`` like open_clip's; neither vocabulary ships offline) or already
    tokenised ids (``{"input_ids", "attention_mask"}`` / an id tensor).  ``max_seq_len`` = the KV-cache window: 1000 by default, the reference's
    (early_fusion_tsfm_models.py:370; its online evaluation runs episodes of 600 steps, 1000 for RoomVisit / ObjectNavMulti), capped at the 1024 keys of the
    single-query attention kernels (csrc/attn_decode.hip) and at the model's ``max_steps``: every step attends to all steps of the episode so far, as the
    reference's llama path does.  Only an episode that outlives that window restarts it, with a warning (the reference's llama caches end at 1000
    steps too)."""

    def __init__(self, model: EarlyFusionCnnTransformer, device="cuda", sampling: str = "greedy", max_seq_len: int = 1000, tokenizer=None,
                 generator: Optional[torch.Generator] = None):
        self._setup(model, device, sampling, max_seq_len, tokenizer, generator)
        self._warned_window = False
        self.reset()

    def _setup(self, model, device, sampling, max_seq_len, tokenizer, generator):
        """What the single and the vector agent share: the checks of the constructor, the KV-cache window, the action list, the tokenizer, eval mode"""
        from .agent import ALL_STRETCH_ACTIONS
        if sampling not in ("greedy", "sample"):
            raise NotImplementedError(f"sampling {sampling!r}: 'greedy' (argmax) or 'sample' (categorical), utils/nn_utils.py sample_action_index_from_logits")
        if getattr(model, "hdim_dec", 64) != 64:
            # the step-by-step agent runs the KV-cached decoder step, which exists for 64-wide heads only (MFMA / decode attention kernels); say so at
            # construction, not at the first get_action.  forward(batch) -- training and offline evaluation -- works for these presets.
            raise NotImplementedError(f"the online agent needs 64-wide decoder heads; this preset has heads of {model.hdim_dec} "
                                      "(TransformerConfig(n, 768, 8): base_6, siglip_base_3_6) -- use forward(batch) on whole windows")
        self.model, self.device, self.sampling, self.max_seq_len = model, torch.device(device), sampling, min(max_seq_len, 1024, model.max_steps)
        self.action_list = list(ALL_STRETCH_ACTIONS)
        self.generator = generator
        if tokenizer is None and model.text_encoder_name == "t5-small":
            from .text import GoalTokenizer
            tokenizer = GoalTokenizer()
        self.tokenizer = tokenizer
        self.model.eval()

    def reset(self):
        self.curr_t = 0
        self.cache = dict()
        self._warned_window = False
        self.model.time_step_counter = 0          # KV-cache slot of the next step; the caches themselves are overwritten slot by slot

    def get_action_list(self):
        return self.action_list

    def _goal(self, goal_spec):
        if isinstance(goal_spec, str):
            if self.tokenizer is None:
                raise ValueError("a string goal needs a tokenizer (SigLIP presets: open_clip's tokenizer is not available offline; pass ids or tokenizer=)")
            if self.model.text_encoder_name == "t5-small":
                enc = self.tokenizer([goal_spec], return_tensors="pt")
                return {k: v.to(self.device) for k, v in enc.items()}
            return torch.as_tensor(self.tokenizer([goal_spec], context_length=64)).to(self.device)
        if isinstance(goal_spec, dict):
            return {k: torch.as_tensor(v).to(self.device).reshape(1, -1) for k, v in goal_spec.items()}
        return torch.as_tensor(goal_spec).to(self.device).reshape(1, -1)

    @torch.no_grad()
    def get_action(self, observations: Dict, goal_spec):
        m, dev = self.model, self.device
        if self.curr_t == 0:
            g = self.cache["goal"] = self._goal(goal_spec)
            self.cache["goal_key"] = goal_ids(g["input_ids"] if isinstance(g, dict) else g)      # (every id, padding included: the key the text features are cached under)
        slot = self.curr_t % self.max_seq_len
        if slot == 0:
            m.time_step_counter = 0
            if self.curr_t > 0 and not self._warned_window:
                # the reference keeps every embedded step and attends to the last max_seq_len of them (a sliding window, :493-495); here the KV cache restarts:
                # the steps right after a restart see a shorter history than the reference's.  time_ids keeps counting like the reference's (:480).
                import warnings
                warnings.warn(f"episode longer than the {self.max_seq_len}-step KV-cache window: the window restarts (the reference slides it)")
                self._warned_window = True
        one = lambda v, dt: torch.as_tensor(np.asarray(v)).to(dev).to(dt).reshape(1, 1)
        batch = {"goals": self.cache["goal"], "time_ids": one(self.curr_t, torch.int64)}      # = curr_t, as early_fusion_tsfm_models.py:480 (not the cache slot)
        # only the model's sensors are read from ``observations`` (early_fusion_tsfm_models.py:410-443)
        if m.has_prev:
            batch["last_actions"] = one(START_TOKEN if self.curr_t == 0 else self.cache["last_actions"], torch.int64)
        if m.has_hand:
            batch["an_object_is_in_hand"] = one(np.asarray(observations.get("an_object_is_in_hand", 0)).reshape(-1)[0], torch.int64)
        for key in m.cameras:
            x = torch.as_tensor(np.ascontiguousarray(observations[key])).to(dev)
            batch[key] = x.reshape((1, 1) + tuple(x.shape))
        prep = m.prepare(batch)
        prep.acting = True                             # a single step against the llama KV caches
        prep.ids_key = self.cache["goal_key"]          # eval mode: the frozen text encoder runs once per episode (the reference caches text_feats at t = 0, :459-465)
        logits, _, _ = m.run_forward(prep, need_grad=False)
        curr = logits.reshape(-1).float()
        probs = torch.softmax(curr, -1)
        idx = int(torch.argmax(curr)) if self.sampling == "greedy" else int(torch.multinomial(probs, 1, generator=self.generator))
        if m.has_prev:                                 # kept only with that sensor (early_fusion_tsfm_models.py:507-508)
            self.cache["last_actions"] = idx
        self.curr_t += 1
        return self.action_list[idx], probs


class EarlyFusionCnnTransformerVectorAgent:
    """``num_episodes`` online episodes of the imitation-learning model behind one set of weights: what ``EarlyFusionCnnTransformerAgent`` does for one episode
    (early_fusion_tsfm_models.py:366-520), for a vector of them that start, end and stall independently -- the evaluation workers of the reference hold one model
    copy each.  ``reset(slot, goal_spec)`` starts an episode in a slot; ``get_actions({slot: observations})`` steps any non-empty subset of the started slots as ONE
    compact batch and returns ``{slot: (action_str, action_probs)}``; slots that are absent keep their cache and their age.

    Every slot owns one row of the llama KV caches and one row of a history of decoder inputs, both rings of W = min(max_seq_len, 1024, model.max_steps) slots
    (``ring_slot``).  Up to W steps an episode takes the KV-cached step: every step attends to the whole episode.  An episode longer than W attends to its last W
    steps, as the reference's agent does (:491-497), without a warning or a restart: from step W on it is decoded anew over the window held in the history ring
    (``Tower._decoder_window_fwd``), because the cached K / V of the decoder layers above the first carry the steps in front of the window in their context -- only
    the first layer's are functions of their own step.  Such a step costs a W-step decoder pass per episode instead of one token's.  Goals of
    different lengths (t5 presets) are right-padded to the longest; the padding is masked in the text encoder and hidden from every fusion layer, so an episode's
    actions do not depend on which other episodes share its batch.  The frozen text encoder reruns only when a ``reset`` brought a new goal.

    The slots' cache rows are the model's: a single agent on the same model writes cache row 0, so run one kind of agent on a model at a time."""

    _setup, _goal, get_action_list = EarlyFusionCnnTransformerAgent._setup, EarlyFusionCnnTransformerAgent._goal, EarlyFusionCnnTransformerAgent.get_action_list

    def __init__(self, model: EarlyFusionCnnTransformer, num_episodes: int, device="cuda", sampling: str = "greedy", max_seq_len: int = 1000, tokenizer=None,
                 generator: Optional[torch.Generator] = None):
        self._slots = EpisodeSlots(num_episodes, START_TOKEN)
        self._setup(model, device, sampling, max_seq_len, tokenizer, generator)
        self.num_episodes = self._slots.num_episodes

    def age(self, slot: int) -> int:
        return self._slots.age(slot)

    def reset(self, slot: int, goal_spec):
        slot = self._slots.slot(slot)
        self._slots.start(slot, goal_ids(self._goal(goal_spec) if isinstance(goal_spec, str) else goal_spec))

    @torch.no_grad()
    def get_actions(self, observations: Dict[int, Dict]) -> Dict[int, tuple]:
        m, dev, sl = self.model, self.device, self._slots
        if not observations:
            raise ValueError("get_actions needs the observations of at least one started slot")
        n, W = len(observations), self.max_seq_len
        # episodes that have outlived their window go last: the model decodes them over the window instead of against the KV ring (stable: the order stays otherwise)
        order = sorted(zip(*sl.rows(observations), observations.values()), key=lambda r: r[1] >= W)
        slots, ages, last, obs = zip(*order)
        t = sl.goal_table(dev, m.text_off, padded=m.text_encoder_name == "t5-small")
        pos, klen = zip(*(ring_slot(a, W) for a in ages))
        # the step's one small upload: cache row (= slot), ring slot to write, slots to read, per row
        rows = torch.tensor([slots, pos, klen], dtype=torch.int32).to(dev)
        col = lambda v, dt: torch.as_tensor(np.asarray(v)).to(dt).reshape(n, 1)
        batch = {"goals": dict(input_ids=t.ids, attention_mask=t.mask), "time_ids": col(ages, torch.int64)}      # the episode's age, as early_fusion_tsfm_models.py:480
        if m.has_prev:
            batch["last_actions"] = col(last, torch.int64)
        if m.has_hand:
            batch["an_object_is_in_hand"] = col([np.asarray(o.get("an_object_is_in_hand", 0)).reshape(-1)[0] for o in obs], torch.int64)
        for cam in m.cameras:
            if torch.is_tensor(obs[0][cam]):
                x = torch.stack([o[cam] for o in obs])
            else:
                x = torch.as_tensor(np.stack([np.asarray(o[cam]) for o in obs]))
            batch[cam] = x.reshape((n, 1) + tuple(x.shape[1:]))
        prep = m.prepare(batch)
        prep.acting = True
        prep.ids_key = t.key                                   # eval mode: the frozen text encoder reruns only when a goal changed
        prep.gid = rows[0]                                     # row -> its slot's goal
        prep.row_cache, prep.row_pos, prep.row_klen = rows[0], rows[1], rows[2]
        prep.row_window, prep.row_slide = W, sum(a >= W for a in ages)
        if t.kvalid is not None and any(t.lens[s] < t.L for s in slots):
            prep.fusion_kvalid = t.kvalid.index_select(0, rows[0])
        m._ensure_caches(self.num_episodes)
        m._ensure_history(self.num_episodes, W)
        logits, _, _ = m.run_forward(prep, need_grad=False)
        probs = torch.softmax(logits.reshape(n, -1).float(), -1)
        idx = torch.argmax(probs, -1) if self.sampling == "greedy" else torch.multinomial(probs, 1, generator=self.generator).reshape(-1)
        out = {}
        for j, (s, i) in enumerate(zip(slots, idx.tolist())):  # the call's one host read
            sl.advance(s, i)
            out[s] = (self.action_list[i], probs[j])
        return out
