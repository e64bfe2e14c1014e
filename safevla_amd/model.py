"""Host mirror of the reference's three-tower actor-critic, running on the gfx950 HIP kernels.

Drop-in surface (same names, argument meaning and state_dict keys as the reference):
  * ``SafeDinoLLAMATxNavActorCriticSeparate.forward(observations, memory, prev_actions, masks)``
        /root/reference/architecture/models/allenact_transformer_models/separate_actor_critic.py:22-37
  * one tower = ``DinoLLAMATxNavActorCritic``   .../allenact_dino_transformer.py:47-475
  * ``DinoTxGoalEncoder``                        .../allenact_dino_transformer.py:478-717
  * llama ``TransformerDecoder``                 /root/reference/training/online/third_party_models/llama/model.py:425-467
  * ``sampler_select``, ``recurrent_memory_specification`` (AllenAct ActorCriticModel API)

MI355X-first design (not a translation of the nn.Module graph):
  * all trainable parameters of the three towers live in ONE flat fp32 arena (plus flat grad / Adam state / bf16
    mirror): a single fused Adam+clip launch, a single RCCL all-reduce, weight-gradient GEMMs accumulate in place;
  * each tower's forward/backward is an explicit kernel schedule over bf16 activations (no autograd tracing inside);
    autograd sees one node per tower, so ``loss.backward()`` of the reference API still works;
  * the frozen T5 text encoder runs once per *unique goal string* (content-hashed on the GPU) instead of once per
    (step, env) row per tower; DINO features are re-laid out once per forward (fp32 channels-first -> bf16 tokens)
    and shared by the three towers.
No CPU / eager fallback: every op below is a C-ABI kernel (include/svla.h); missing library => import error.
"""
import contextlib
import math
import os
from typing import Dict, List, Optional, Tuple

import numpy as np

import torch
import torch.nn as nn

from . import ops
from .api import CategoricalDistr, SafeActorCriticOutput
from .losses import HLGaussLoss
from .text import GoalTokenizer, bytes_to_str

N_ACTIONS = 20
D = 512
DINO = 384
NPATCH = 84          # 7 x 12 grid per camera
TEXT_OFF = 1 + 2 * NPATCH        # text offset of the two-camera set; a tower's own is ``Tower.text_off`` = 1 + ncam * NPATCH
CAMERAS = ("raw_navigation_camera", "raw_manipulation_camera")      # the camera sensors that are built, in the order of their fusion tokens
NON_VISUAL_SENSORS = ("last_actions", "an_object_is_in_hand")
MAX_ACTING_WINDOW = 1024          # keys of the single-query attention kernels = longest KV-cache window (max_steps) of the acting step
TEXT_ENCODER_DIMS = {"t5-small": 512, "SigLIPBase": 768, "SigLIPLarge": 1024}
BF16, F32 = torch.bfloat16, torch.float32
SEED_STEP = 0x3C6EF35             # what the device-resident dropout seed of a recorded / captured pass advances by per pass (Tower.advance_device_seed, svla_acting_stage)
_NO_COMPRESSOR_BITS = os.environ.get("SVLA_NO_COMPRESSOR_BITS", "0") == "1"     # A/B switch of the 1-bit compressor ReLU masks
MAX_TILE_SEQ = 512                # keys of the tile kernels of csrc/attn.hip and of every attention backward: longer sequences are forward only (csrc/attn_seq_long.hip)
# A/B switch of Tower._decoder_window_fwd (tools/ab_attn_causal_long.py, tests): True keeps windows above MAX_TILE_SEQ steps on one single-query row per (episode,
# position) instead of the streaming causal kernel.  Read once from SVLA_WINDOW_DECODE_ROWS; a module flag afterwards.
WINDOW_DECODE_ROWS = os.environ.get("SVLA_WINDOW_DECODE_ROWS", "0") == "1"


class _NS(nn.Module):
    """bare namespace module (parameters are attached by the arena)"""


def _seq(n):
    return nn.Sequential(*[_NS() for _ in range(n)])


# ================================================================================================ parameter arena
class _Arena:
    """Flat fp32 parameter arena shared by the three towers."""

    def __init__(self):
        self.specs: List[Tuple[nn.Module, str, Tuple[int, ...], str]] = []
        self.offsets: Dict[int, Tuple[int, int]] = {}
        self._tower_starts: List[int] = []

    def declare(self, owner: nn.Module, name: str, shape, init: str):
        self.specs.append((owner, name, tuple(shape), init))

    def begin_tower(self, align: int = 256):
        """Start a new tower's contiguous range on an ``align``-element boundary (16-byte aligned bf16 weight views for the LDS-DMA
        loads of every tower -- one tower has an odd number of trainable elements -- and per-tower all-reduce / Adam ranges)."""
        n = sum(int(np.prod(s[2])) for s in self.specs)
        pad = (-n) % align
        if pad:
            self.specs.append((None, "_pad", (pad,), "zeros"))
        self._tower_starts.append(n + pad)

    def build(self, device):
        total = sum(int(np.prod(s[2])) for s in self.specs)
        total += (-total) % 256
        starts = self._tower_starts or [0]
        self.tower_ranges = [(a, b) for a, b in zip(starts, starts[1:] + [total])]
        self.total = total
        self.flat_p = torch.zeros(total, device=device, dtype=F32)
        self.flat_g = torch.zeros(total, device=device, dtype=F32)
        self.flat_m = torch.zeros(total, device=device, dtype=F32)
        self.flat_v = torch.zeros(total, device=device, dtype=F32)
        self.flat_bf16 = torch.zeros(total, device=device, dtype=BF16)
        off = 0
        g = torch.Generator().manual_seed(0)
        for owner, name, shape, init in self.specs:
            n = int(np.prod(shape))
            if owner is None:        # alignment padding: stays zero (zero gradient => Adam never moves it)
                off += n
                continue
            view = self.flat_p[off:off + n].view(shape)
            view.copy_(_init_tensor(shape, init, g).to(device))
            p = nn.Parameter(view, requires_grad=True)
            p.grad = self.flat_g[off:off + n].view(shape)
            setattr(owner, name, p)
            self.offsets[id(p)] = (off, n)
            off += n

    def slab(self, p: nn.Parameter, flat: torch.Tensor, shape=None):
        off, n = self.offsets[id(p)]
        return flat[off:off + n].view(shape if shape is not None else p.shape)


def _init_tensor(shape, init, g):
    if init == "ones":
        return torch.ones(shape)
    if init == "zeros":
        return torch.zeros(shape)
    if init == "tok":
        return 0.1 * torch.rand(shape, generator=g)
    if init == "emb":
        return (torch.rand(shape, generator=g) * 2 - 1) * 0.01
    if init == "lin":
        fan_in = int(np.prod(shape[1:]))
        return (torch.rand(shape, generator=g) * 2 - 1) / math.sqrt(fan_in)
    if init == "actor":
        w = torch.empty(shape)
        nn.init.orthogonal_(w, gain=0.01)
        return w
    if init == "critic":
        w = torch.empty(shape)
        nn.init.orthogonal_(w)
        return w
    raise KeyError(init)


# ================================================================================================ one tower
def sensor_set(input_sensors):
    """``input_sensors`` of the reference's constructors -> (cameras in fusion order, in-hand sensor?, previous action embedded?).  An unknown name is a ValueError that
    lists what is built: the bbox sensors, ``relative_arm_location_metadata`` and the duplicate cameras of utils/sensor_constant_utils.py are not."""
    names = list(input_sensors)
    unknown = [n for n in names if n not in CAMERAS + NON_VISUAL_SENSORS]
    if unknown:
        raise ValueError(f"input sensors {unknown} are not built; built are {list(CAMERAS + NON_VISUAL_SENSORS)}")
    cameras = tuple(c for c in CAMERAS if c in names)
    if not cameras:
        raise ValueError(f"input sensors {names} hold no camera; a model needs a non-empty subset of {list(CAMERAS)}")
    return cameras, "an_object_is_in_hand" in names, "last_actions" in names


class Tower(nn.Module):
    """``DinoLLAMATxNavActorCritic`` (dinov2_vits_tsfm_base.py:234-270) over a sensor set: ``cameras`` (a non-empty subset of ``CAMERAS``), ``in_hand`` (the
    an_object_is_in_hand embedding) and ``prev_actions`` (the previous-action embedding) -- what the reference's constructors take as uuids that may be None
    (allenact_dino_transformer.py:67-68,129-132,517-527) and as ``input_sensors`` (early_fusion_tsfm_models.py:90-102).  Defaults: the full four-sensor set.
    A sensor that is absent has no parameter in the arena (and no name in ``state_dict()``), no tokens in the fusion sequence and no term in the decoder input."""

    def __init__(self, arena: _Arena, device, n_fusion_layers=3, n_decoder_layers=3, max_steps=500, critic_type="linear",
                 precision="bf16", dino_dim=DINO, text_encoder="t5-small", d_model=512, n_heads=8, n_heads_decoder=None,
                 cameras=CAMERAS, in_hand=True, prev_actions=True):
        super().__init__()
        self.cameras = tuple(c for c in CAMERAS if c in tuple(cameras))
        if not self.cameras or len(self.cameras) != len(tuple(cameras)):
            raise ValueError(f"cameras {list(cameras)}: a non-empty subset of {list(CAMERAS)} without repeats")
        self.has_hand, self.has_prev = bool(in_hand), bool(prev_actions)
        # fusion sequence of one row: [fusion token | ncam x 84 camera tokens | L text tokens] (text_cond_visual_encoder.py:203-219)
        self.ncam = len(self.cameras)
        self.text_off = 1 + self.ncam * NPATCH
        # transformer width of the fusion encoder AND the decoder (512 x 8 heads everywhere in the RL towers, allenact_dino_transformer.py:101-117; the imitation-
        # learning presets also use 768 x 12, early_fusion_tsfm_models.py:275-294); llama's SwiGLU hidden size follows from it (llama_model.py:330-334)
        n_heads_decoder = n_heads if n_heads_decoder is None else n_heads_decoder
        if d_model % 64 or d_model > 1024 or d_model % n_heads or d_model % n_heads_decoder or max(d_model // n_heads, d_model // n_heads_decoder) > 128:
            raise NotImplementedError(f"transformer width {d_model} with {n_heads} / {n_heads_decoder} heads")
        D = self.D = d_model
        H = self.H = n_heads                      # fusion transformer (nn.TransformerEncoderLayer nhead)
        self.Hdec = n_heads_decoder               # llama decoder (ModelArgs.n_heads); TransformerConfig(3, 768, 8) + TransformerConfig(6, 768, 12) = siglip_base_3_6
        # head widths: 64 and 96 (= 768 / 8: base_6, siglip_base_3_6) on the MFMA attention kernels (csrc/attn.hip, csrc/attn_hd96.hip); any other width takes the
        # fp32 attention kernels through fp32 copies of the operands (ops.attn_fwd: a slow path)
        self.hdim, self.hdim_dec = d_model // n_heads, d_model // n_heads_decoder
        HD = self.dec_hidden = 256 * ((int(2 * 4 * d_model / 3) + 255) // 256)
        F = self.dff = 2048               # feed-forward width of the fusion layers: nn.TransformerEncoderLayer's default, as the reference uses it
        self.dino_dim = dino_dim          # channel width of the frozen image features: 384 (ViT-S/14), 768 (ViT-B/14, SigLIP-B), 1024 (ViT-L), 2048 (CLIP RN50)
        # frozen text encoder and the width of its features (text_cond_visual_encoder.py:24-45 ``TEXT_ENCODER_DIMS`` / ``create_text_encoder``): the RL towers
        # and the t5 presets of the IL model use t5-small; the IL model's ``siglip_*`` presets the SigLIP text tower (tokens + pooled token, siglip_text.py)
        if text_encoder not in TEXT_ENCODER_DIMS:
            raise NotImplementedError("Only SigLIP and T5 text encoders are supported.")
        self.text_encoder_name, self.text_dim = text_encoder, TEXT_ENCODER_DIMS[text_encoder]
        if precision not in ("bf16", "fp32"):
            raise ValueError(f"precision must be 'bf16' (MFMA product path) or 'fp32' (verification mode), got {precision!r}")
        # activation / GEMM-operand dtype.  "fp32" = the verification mode: the same schedule on the fp32 twins of every kernel
        # (include/svla.h, last section), for comparing with the reference's fp32 arithmetic at fp32 tolerance; not a fast path.
        self.precision, self.adt = precision, (F32 if precision == "fp32" else BF16)
        if critic_type not in ("linear", "mlp", "discrete"):
            print(f"Unknown critic type: {critic_type}")
            raise NotImplementedError
        self.critic_type = critic_type
        self.arena = arena
        self.device_ = device
        if not 1 <= int(max_steps) <= MAX_ACTING_WINDOW:
            # the KV-cache window of the acting step: the single-query attention kernels end at 1024 keys (csrc/attn_decode.hip; the reference's policies and
            # llama caches are built for 1000).  Refused here, not by a kernel status at step 1024 -- or, on the recorded path (S = max_steps), at the first step
            raise ValueError(f"max_steps = {max_steps}: the KV-cache window of the acting step is limited to {MAX_ACTING_WINDOW} steps")
        self.max_steps = max_steps
        self.time_step_counter = 0
        self.prune_last = True      # dead-output elimination in the last fusion layer (exact; see _fusion_layer_fwd)
        # pruned last layer of an update pass: K / V projections absorbed into its single query, K and V never materialised (csrc/attn_q1.hip; _fusion_layer_fwd).
        # SVLA_LAST_LAYER_KV=1 keeps the materialised K / V path (A/B)
        self.absorb_last = os.environ.get("SVLA_LAST_LAYER_KV", "0") != "1"
        # BASELINE config 5 ("fp8 MFMA attention"): the full-sequence fusion-encoder attention layers run on the e4m3 / e5m2 kernels
        # (svla_attn_fp8_*); the pruned last layer (one query per row) and the decoder keep the bf16 kernels.  bf16 precision only.
        self.fp8_attention = False
        # The reference leaves the policy in train() mode (allenact_dino_transformer.py:193): nn.TransformerEncoderLayer's
        # dropout 0.1 is active in rollouts and updates.  Same here: ``.eval()`` turns it off (parity fixtures are eval-mode).
        self.dropout_p = 0.1
        self.t5_dropout = True      # the frozen text encoder's own dropout (also active in the reference's train mode)
        self.drop_seed_base = 0x5AFE + 977 * len(arena.specs)   # distinct per tower; settable for reproducible tests
        self._fwd_count = 0
        # acting path: llama KV caches (+ version: recorded steps hold pointers into them), eval-mode text-feature cache, gamma-folded decoder weights (refresh_folded), norm-fused
        # GEMMs in the acting step's decoder / the frozen text encoder (None: by size).  Below: step counter, dropout seed, step indices of recorded / captured passes (device memory)
        self._kv, self._kv_version, self._t5_cache, self._wg, self._wg_dirty, self.rms_fused, self.t5_fused = None, 0, (None, None), {}, True, True, None
        self._t_dev = self._seed_dev = self._seed_dev_buf = self._ar_steps = self._last_full_logits = self._hist = None
        dec = arena.declare
        ve = self.visual_encoder = _NS()
        dec(ve, "fusion_token", (D,), "tok")
        for cam in self.cameras:                                            # adjacent: [ncam, D] camera-token table
            dec(ve, f"visual_sensor_token_{cam}", (D,), "tok")
        ve.text_adapter = _seq(3)
        dec(ve.text_adapter[0], "weight", (D, self.text_dim), "lin"); dec(ve.text_adapter[0], "bias", (D,), "zeros")
        dec(ve.text_adapter[1], "weight", (D,), "ones"); dec(ve.text_adapter[1], "bias", (D,), "zeros")
        ve.visual_compressor = _seq(4)
        dec(ve.visual_compressor[0], "weight", (D, dino_dim, 1, 1), "lin"); dec(ve.visual_compressor[0], "bias", (D,), "zeros")
        dec(ve.visual_compressor[2], "weight", (D, D, 1, 1), "lin"); dec(ve.visual_compressor[2], "bias", (D,), "zeros")
        ve.visual_adapter = _seq(3)
        dec(ve.visual_adapter[0], "weight", (D, D), "lin"); dec(ve.visual_adapter[0], "bias", (D,), "zeros")
        dec(ve.visual_adapter[1], "weight", (D,), "ones"); dec(ve.visual_adapter[1], "bias", (D,), "zeros")
        ve.fusion_xformer = _NS()
        ve.fusion_xformer.layers = nn.ModuleList()
        for _ in range(n_fusion_layers):
            l = _NS()
            l.self_attn = _NS()
            dec(l.self_attn, "in_proj_weight", (3 * D, D), "lin"); dec(l.self_attn, "in_proj_bias", (3 * D,), "zeros")
            l.self_attn.out_proj = _NS()
            dec(l.self_attn.out_proj, "weight", (D, D), "lin"); dec(l.self_attn.out_proj, "bias", (D,), "zeros")
            l.linear1 = _NS(); dec(l.linear1, "weight", (F, D), "lin"); dec(l.linear1, "bias", (F,), "zeros")
            l.linear2 = _NS(); dec(l.linear2, "weight", (D, F), "lin"); dec(l.linear2, "bias", (D,), "zeros")
            l.norm1 = _NS(); dec(l.norm1, "weight", (D,), "ones"); dec(l.norm1, "bias", (D,), "zeros")
            l.norm2 = _NS(); dec(l.norm2, "weight", (D,), "ones"); dec(l.norm2, "bias", (D,), "zeros")
            ve.fusion_xformer.layers.append(l)
        if text_encoder == "t5-small":
            ve.text_encoder = T5Frozen(device)
        else:
            from .siglip_text import SIGLIP_TEXT_PRESETS, SigLIPTextFrozen
            ve.text_encoder = SigLIPTextFrozen(device, **SIGLIP_TEXT_PRESETS[text_encoder])
        if self.has_hand:
            self.object_in_hand_embed = _NS(); dec(self.object_in_hand_embed, "weight", (3, D), "emb")
        if self.has_prev:
            self.last_actions_embed = _NS(); dec(self.last_actions_embed, "weight", (N_ACTIONS + 2, D), "emb")
        self.time_encoder = _NS()
        self.time_encoder.register_buffer("div_term", torch.exp(torch.arange(0, D, 2) * (-math.log(10000.0) / D)).to(device))
        self.decoder = _NS()
        self.decoder.layers = nn.ModuleList()
        for _ in range(n_decoder_layers):
            l = _NS()
            l.attention = _NS()
            for n in ("wq", "wk", "wv"):                                   # adjacent: fused [3 D, D] QKV weight
                setattr(l.attention, n, _NS()); dec(getattr(l.attention, n), "weight", (D, D), "lin")
            l.attention.wo = _NS(); dec(l.attention.wo, "weight", (D, D), "lin")
            l.feed_forward = _NS()
            l.feed_forward.w1 = _NS(); l.feed_forward.w2 = _NS(); l.feed_forward.w3 = _NS()
            dec(l.feed_forward.w1, "weight", (HD, D), "lin")             # w1, w3 adjacent: fused [2 HD, D]
            dec(l.feed_forward.w3, "weight", (HD, D), "lin")
            dec(l.feed_forward.w2, "weight", (D, HD), "lin")
            l.attention_norm = _NS(); dec(l.attention_norm, "weight", (D,), "ones")
            l.ffn_norm = _NS(); dec(l.ffn_norm, "weight", (D,), "ones")
            self.decoder.layers.append(l)
        self.decoder.norm = _NS(); dec(self.decoder.norm, "weight", (D,), "ones")
        self.decoder.output = _NS(); dec(self.decoder.output, "weight", (D, D), "lin")
        self.actor = _NS(); self.actor.linear = _NS()
        dec(self.actor.linear, "weight", (N_ACTIONS, D), "actor"); dec(self.actor.linear, "bias", (N_ACTIONS,), "zeros")
        # critic heads of allenact_dino_transformer.py:147-162 (LinearCriticHead [3P] / MLPCriticHead :720-740 / DiscreteCriticHead :743-766)
        self.critic = _NS()
        if critic_type == "linear":
            self.critic.fc = _NS()
            dec(self.critic.fc, "weight", (1, D), "critic"); dec(self.critic.fc, "bias", (1,), "zeros")
            self._head_dims = []
        else:
            dims = [D, 256, 101] if critic_type == "discrete" else [D, 256, 256, 1]
            self.critic.fc = _seq(2 * (len(dims) - 1) - 1)              # Linear, ReLU, Linear[, ReLU, Linear]: state_dict keys fc.0 / fc.2 [/ fc.4]
            for j in range(len(dims) - 1):
                dec(self.critic.fc[2 * j], "weight", (dims[j + 1], dims[j]), "critic"); dec(self.critic.fc[2 * j], "bias", (dims[j + 1],), "zeros")
            self._head_dims = dims
            if critic_type == "discrete":   # "bins = 101 ... -5 to 15 ... sigma=0.15" (:152-156)
                self.critic.loss_fn = HLGaussLoss(min_value=-5.0, max_value=15.0, num_bins=101, sigma=0.15)
        self._wt: Dict[str, torch.Tensor] = {}

    # ---- weight views -------------------------------------------------------------------------------------
    def _gemm_weights(self):
        """(key, parameter(s), [N, K]) for every MFMA GEMM weight of the tower."""
        D, H, HD = self.D, self.H, self.dec_hidden
        ve = self.visual_encoder
        out = [("c1", [ve.visual_compressor[0].weight], (D, self.dino_dim)), ("c2", [ve.visual_compressor[2].weight], (D, D)),
               ("va", [ve.visual_adapter[0].weight], (D, D)), ("ta", [ve.text_adapter[0].weight], (D, self.text_dim))]
        for i, l in enumerate(ve.fusion_xformer.layers):
            out += [(f"f{i}.in", [l.self_attn.in_proj_weight], (3 * D, D)), (f"f{i}.out", [l.self_attn.out_proj.weight], (D, D)),
                    (f"f{i}.l1", [l.linear1.weight], (self.dff, D)), (f"f{i}.l2", [l.linear2.weight], (D, self.dff))]
        for i, l in enumerate(self.decoder.layers):
            a, f = l.attention, l.feed_forward
            out += [(f"d{i}.qkv", [a.wq.weight, a.wk.weight, a.wv.weight], (3 * D, D)), (f"d{i}.wo", [a.wo.weight], (D, D)),
                    (f"d{i}.w13", [f.w1.weight, f.w3.weight], (2 * HD, D)), (f"d{i}.w2", [f.w2.weight], (D, HD))]
        out.append(("dout", [self.decoder.output.weight], (D, D)))
        return out

    def bind(self):
        """Create bf16 / fp32-grad views into the arena (call once after arena.build)."""
        D, H, HD = self.D, self.H, self.dec_hidden
        ar = self.arena
        self._w, self._dw = {}, {}
        for key, ps, (n, k) in self._gemm_weights():
            off, _ = ar.offsets[id(ps[0])]
            self._w[key] = (ar.flat_p if self.adt == F32 else ar.flat_bf16)[off:off + n * k].view(n, k)
            self._dw[key] = ar.flat_g[off:off + n * k].view(n, k)
            self._wt[key] = torch.empty(k, n, device=self.device_, dtype=self.adt)
        ve = self.visual_encoder
        off, _ = ar.offsets[id(getattr(ve, f"visual_sensor_token_{self.cameras[0]}"))]
        self._camtok = ar.flat_p[off:off + self.ncam * D].view(self.ncam, D)
        self._dcamtok = ar.flat_g[off:off + self.ncam * D].view(self.ncam, D)

    def refresh_transposes(self):
        ar = self.arena
        for key, ps, (n, k) in self._gemm_weights():
            off, _ = ar.offsets[id(ps[0])]
            ops.transpose_cast_bf16(ar.flat_p[off:off + n * k].view(n, k), self._wt[key])
        self._wg_dirty = True

    def refresh_folded(self):
        """W * gamma[None, :] (bf16) of the llama decoder's pre-norm linears -- RMSNorm(x) @ W^T = rstd(x) * (x @ (W gamma)^T) -- for the acting step's norm-fused
        GEMMs (ops.gemm_nt_rmsa).  Persistent buffers refreshed IN PLACE (recorded acting steps hold their addresses), lazily: only an acting step after an
        optimiser step / load_state_dict pays for it."""
        D, H, HD = self.D, self.H, self.dec_hidden
        if self.adt != BF16 or not self._wg_dirty:
            return
        ar = self.arena
        for i, l in enumerate(self.decoder.layers):
            a, f = l.attention, l.feed_forward
            for key, first, n, gamma in ((f"d{i}.qkv", a.wq.weight, 3 * D, l.attention_norm.weight), (f"d{i}.w13", f.w1.weight, 2 * HD, l.ffn_norm.weight)):
                off, _ = ar.offsets[id(first)]
                w32 = ar.flat_p[off:off + n * D].view(n, D)
                if key not in self._wg:
                    self._wg[key] = torch.empty(n, D, device=self.device_, dtype=BF16)
                self._wg[key].copy_(w32 * gamma.detach().float()[None, :])
        self._wg_dirty = False

    def _drop_sites(self):
        """Dropout descriptors of one forward pass: site(layer, k), k = 0 attention probabilities, 1 attention sub-layer output,
        2 feed-forward activation, 3 feed-forward sub-layer output; None in eval mode.  The pass seed is saved with the
        activations so that the backward regenerates the same masks."""
        if not self.training or self.dropout_p <= 0:
            return None, (lambda i, k, rm=1: None)
        self._fwd_count += 1
        seed = (self.drop_seed_base * 0x9E3779B1 + self._fwd_count * 0x85EBCA77) & 0xFFFFFFFF
        return seed, self._site_fn(seed)

    def _site_fn(self, seed):
        p = self.dropout_p
        sd = self._seed_dev      # captured acting graph: the pass seed lives in device memory (fresh noise per replay)
        return (lambda i, k, rm=1: ops.Dropout(seed, 4 * i + k, p, rm, seed_dev=sd)) if seed is not None else (lambda i, k, rm=1: None)

    def g(self, p):  # fp32 grad view of a parameter
        return self.arena.slab(p, self.arena.flat_g)

    # ---- acting path state (llama KV caches, llama/model.py:224-247; counter semantics allenact_dino_transformer.py:376-406)
    def _ensure_caches(self, B: int):
        if self._kv is None or self._kv[0].shape[0] < B:
            self._kv_version += 1        # recorded steps hold pointers into the caches: new caches, new plans
            self._kv = [torch.zeros(B, self.max_steps, 2 * self.D, device=self.device_, dtype=self.adt) for _ in self.decoder.layers]

    def _ensure_history(self, n: int, window: int):
        """decoder inputs of the last ``window`` steps of ``n`` episodes (vector steps with ``Prep.row_window``: ``_decoder_rows_fwd``)"""
        if self._hist is None or self._hist.shape[0] < n or self._hist.shape[1] != window:
            self._hist = torch.zeros(n, window, self.D, device=self.device_, dtype=self.adt)

    def cache_select(self, keep: list):
        if self._kv is not None:
            idx = torch.as_tensor(keep, device=self.device_, dtype=torch.long)
            self._kv = [c[idx].contiguous() for c in self._kv]
            self._kv_version += 1

    # ---- dropout seed of recorded / captured passes: in device memory, read when a kernel starts, so every replay draws fresh noise
    def advance_device_seed(self):
        """once before every recorded, captured or replayed pass (its forward and backward read the same seed); wraps in int32"""
        if self._seed_dev_buf is None:      # created on first use
            self._seed_dev_buf = torch.tensor([(self.drop_seed_base * 0x9E3779B1) & 0x7FFFFFFF], device=self.device_, dtype=torch.int32)
        self._seed_dev_buf.add_(SEED_STEP)

    @contextlib.contextmanager
    def device_resident(self, t_dev=None):
        """Inside, no kernel argument depends on the step (recording, capture): dropout descriptors point at the device seed, acting steps read the counter ``t_dev``."""
        self._t_dev, self._seed_dev = t_dev, self._seed_dev_buf
        try:
            yield
        finally:
            self._t_dev = self._seed_dev = None

    def static_step(self, st: "_ActingState"):
        """One acting forward on the static buffers of ``st`` in the step-independent form -> (logits, values); the wrapper advances the host counter once per step."""
        keep = self.time_step_counter
        with self.device_resident(st.t_dev):
            logits, values, _ = self.run_forward(st, need_grad=False)
        self.time_step_counter = keep
        return logits, values

    # ---- forward: a driver over one method per stage ---------------------------------------------------------------------------
    def run_forward(self, prep: "Prep", need_grad: bool):
        """-> logits [T, B, A], values [T, B, 1], the saved activations for ``run_backward`` (opaque to callers; None without ``need_grad``)"""
        D, T, B, S = self.D, prep.T, prep.B, prep.S
        self._check_seq_len(T, need_grad)
        per_row = prep.row_pos is not None
        if per_row and (T > 1 or need_grad or not prep.acting or prep.row_klen is None):
            raise ValueError("row_pos / row_klen: the acting step on per-row KV rings is a T = 1 forward without gradients, with both fields given")
        if prep.fusion_kvalid is not None and (need_grad or self.fp8_attention):
            raise ValueError("fusion_kvalid: the key-padding mask of the fusion encoder exists in the bf16 / fp32 forward only (no backward, no fp8 form)")
        ragged = prep.row_map is not None
        if ragged and (prep.acting or per_row or prep.fusion_kvalid is not None or self.fp8_attention or self.adt != BF16 or prep.row_inv is None or prep.row_seg is None):
            raise ValueError("row_map: compact fusion rows exist for forward(batch) on the bf16 path (no acting step, fusion_kvalid, fp8_attention or fp32 mode), "
                             "with row_inv and row_seg given")
        if not per_row and (T > 1 or need_grad or not prep.acting or self.time_step_counter >= self.max_steps):
            self.time_step_counter = 0
        seed, site = self._drop_sites()
        c = dict(drop_seed=seed, fusion=[])  # saved activations
        xf = self._inputs_fwd(prep, c, need_grad)
        nfl = len(self.visual_encoder.fusion_xformer.layers)
        for i in range(nfl):
            xf, saved = self._fusion_layer_fwd(i, xf, prep, site, need_grad)
            if need_grad:
                c["fusion"].append(saved)
        # decoder over the rollout time axis, rows (b*T + t); a pruned last fusion layer left the position-0 rows only
        xd = torch.empty(prep.R, D, device=self.device_, dtype=self.adt)
        ldx, x0 = (D if nfl and self.prune_last else S * D), xf
        if ragged:
            # compact rows -> decoder-row order (t * B + b); a padded step gets a zero feature, its embedding terms are added below as usual
            x0, es = torch.empty(prep.R, D, device=self.device_, dtype=self.adt), xf.element_size()
            ops.rows_gather(x0, D * es, xf, ldx * es, prep.row_map, prep.R, D * es, prep.Rf)
            ldx = D
        # an absent sensor's table and indices go in as None together (svla_decoder_embed_fwd: the term is skipped)
        ops.decoder_embed_fwd(x0, ldx, self.last_actions_embed.weight if self.has_prev else None,
                              self.object_in_hand_embed.weight if self.has_hand else None, self.time_encoder.div_term,
                              prep.prev_actions if self.has_prev else None, prep.masks if self.has_prev else None, prep.hand if self.has_hand else None,
                              prep.time_step, T, B, xd)
        if T == 1 and not need_grad and prep.acting:
            # acting: one new token per env against the KV cache.  A one-step UPDATE batch (need_grad) takes the sequence form -- a sequence of length one has no
            # history to attend to, and the backward needs the saved activations -- and so does a batch whose Prep says ``acting = False`` (the imitation-learning
            # model's ``forward(batch)`` on one-step windows: independent sequences, never the cache of an earlier call; its online agent sets ``acting = True``)
            xd, c["dec"] = (self._decoder_rows_fwd(xd, prep) if per_row else self._decoder_step_fwd(xd, prep)), []
        else:
            xd, c["dec"] = self._decoder_seq_fwd(xd, prep, need_grad)
        logits, values = self._heads_fwd(xd, prep, c, need_grad)
        c["xf_last"] = xf
        return logits.view(T, B, N_ACTIONS), values.view(T, B, 1), (c if need_grad else None)

    def _inputs_fwd(self, prep, c, need_grad):
        """Visual compressor + adapter (all cameras), frozen text encoder + text adapter, ``fusion_fill`` -> the fusion transformer's input rows [R * S, D]"""
        D, R, S, L, U, ve, w = self.D, prep.Rf, prep.S, prep.L, prep.U, self.visual_encoder, self._w      # R: fusion rows (all decoder rows, or the valid steps only)
        if S != self.text_off + L or prep.tokens.numel() != R * self.ncam * NPATCH * self.dino_dim:
            raise ValueError(f"inputs of {prep.tokens.numel() // max(R * NPATCH * self.dino_dim, 1)} camera(s), S = {S} for a tower of {self.ncam} camera(s), S = {self.text_off + L}")
        M2 = R * self.ncam * NPATCH
        tok = prep.tokens.view(M2, self.dino_dim)
        # ReLU derivatives of the two compressor convs as 1 bit per element (like the feed-forward's): the input-gradient GEMMs then read
        # M2 x 64 mask bytes instead of re-reading a whole M2 x 512 bf16 activation
        bits = need_grad and self.adt == BF16 and not _NO_COMPRESSOR_BITS
        c1b, c2b = (torch.empty(ops.relu_bits_bytes(M2, D), device=self.device_, dtype=torch.uint8) if bits else None for _ in range(2))
        c1 = ops.gemm_nt(tok, w["c1"], M2, D, self.dino_dim, bias=ve.visual_compressor[0].bias, act=ops.ACT_RELU, relu_bits_out=c1b)
        c2 = ops.gemm_nt(c1, w["c2"], M2, D, D, bias=ve.visual_compressor[2].bias, act=ops.ACT_RELU, relu_bits_out=c2b)
        a1 = ops.gemm_nt(c2, w["va"], M2, D, D, bias=ve.visual_adapter[0].bias)
        x = torch.empty(R, S, D, device=self.device_, dtype=self.adt)
        _, va_mean, va_rstd = ops.norm_fwd(a1, ve.visual_adapter[1].weight, ve.visual_adapter[1].bias, 1e-5, M2, relu=True,
                                           tok=self._camtok, tok_group=NPATCH, y=x, ymap=(self.ncam * NPATCH, S, 1), D=D)
        t5_seed, key = (c["drop_seed"] if self.t5_dropout else None), prep.ids_key
        if t5_seed is None and key is not None and self._t5_cache[0] == key:
            t5 = self._t5_cache[1]     # eval mode: the frozen encoder is a pure function of the goal tokens (one episode = one goal)
        else:
            t5 = ve.text_encoder.encode(prep.ids, prep.attn_mask_u8 if prep.attn_mask_u8 is not None else prep.attn_mask, drop_seed=t5_seed, drop_p=self.dropout_p,
                                        dtype=self.adt, seed_dev=self._seed_dev, fused=self.t5_fused)   # [U*L, text_dim], frozen (SigLIP: ids are [U, L - 1], the pooled token is row L - 1)
            self._t5_cache = (key, t5) if (t5_seed is None and key is not None) else (None, None)
        ta = ops.gemm_nt(t5, w["ta"], U * L, D, self.text_dim, bias=ve.text_adapter[0].bias)
        tf, ta_mean, ta_rstd = ops.norm_fwd(ta, ve.text_adapter[1].weight, ve.text_adapter[1].bias, 1e-5, U * L, relu=True, D=D)
        ops.fusion_fill(ve.fusion_token, tf, prep.gid, x, R, S, L, self.text_off)
        c.update(c1=c1, c2=c2, c1b=c1b, c2b=c2b, a1=a1, va=(va_mean, va_rstd), t5=t5, ta=ta, ta_stats=(ta_mean, ta_rstd))
        return x.view(R * S, D)

    def _fusion_layer_fwd(self, i, xf, prep, site, need_grad):
        """Fusion layer ``i`` on the token rows ``xf`` [R * S, D] -> (output rows, saved activations or None).  Its attention half has four forms (absorbed single
        query, single query over materialised K / V, fp8, full QKV) that meet at ``ao``; the rest of the layer is ``_fusion_post_fwd``."""
        D, H, R, S, w, SCF = self.D, self.H, prep.Rf, prep.S, self._w, self.hdim ** -0.5         # SCF: 0.125 for 64-wide heads; R: fusion rows
        M, l = R * S, self.visual_encoder.fusion_xformer.layers[i]
        if self.prune_last and i == len(self.visual_encoder.fusion_xformer.layers) - 1:
            # Only sequence position 0 of the last fusion layer is consumed (allenact_dino_transformer.py:708 x[:, 0]): Q / attention / out_proj / norm1 / FFN /
            # norm2 run on the R position-0 rows only; K/V still cover all tokens (projected in full, or absorbed into the query: below).  Identical outputs and
            # gradients; ~84 % less work in this layer.
            b_in = l.self_attn.in_proj_bias
            q0 = ops.gemm_nt(xf, w[f"f{i}.in"][:D], R, D, D, bias=b_in[:D], lda=S * D)
            # Update passes on the bf16 path: with one query per (row, head) the K and V projections move onto the query side exactly --
            # qt_h = W_k,h^T q_h scores the raw tokens (the K bias shifts every score of a head alike: the softmax drops it), c_h = sum_j pd_hj x_j,
            # o_h = W_v,h c_h + (sum_j pd_hj) b_v,h -- so K / V for all M tokens are never computed or kept.  The per-head products are plain GEMMs over
            # head-expanded [8 R, 512] rows.  Acting steps, fp32 verification mode and absorb_last = False take the materialised branch below.
            if need_grad and self.absorb_last and self.adt == BF16 and self.hdim == 64 and H == 8 and S <= 256:
                eq, _, _ = ops.head_expand(q0, R)
                qt = ops.gemm_nt(eq, self._wt[f"f{i}.in"][:, D:2 * D], 8 * R, D, D)
                cc, sig, prob = ops.attn_q1_fwd(xf, S * D, qt, R, S, SCF, drop=site(i, 0))
                ao = ops.head_pick(ops.gemm_nt(cc, w[f"f{i}.in"][2 * D:], 8 * R, D, D), R, sigma=sig, bias=b_in[2 * D:])
                att = dict(absorbed=True, eq=eq, qt=qt, cc=cc, sig=sig, prob=prob)
            else:
                kv = ops.gemm_nt(xf, w[f"f{i}.in"][D:], M, 2 * D, D, bias=b_in[D:])
                ao, lse = ops.attn_fwd(q0, kv, kv[:, D:], 2 * D, R, S, H, SCF, kvalid=prep.fusion_kvalid, save_lse=need_grad, Sq=1, ldq=D, drop=site(i, 0),
                                       head_dim=self.hdim)
                att = dict(absorbed=False, kv=kv, lse=lse)
            xo, post = self._fusion_post_fwd(i, ao, R, xf, S * D, S, False, site, need_grad)
            return xo, (dict(pruned=True, x=xf, q0=q0, ao=ao, **att, **post) if need_grad else None)
        qkv = ops.gemm_nt(xf, w[f"f{i}.in"], M, 3 * D, D, bias=l.self_attn.in_proj_bias)
        f8 = None
        if self.fp8_attention and self.adt == BF16 and S <= 256 and self.hdim == 64:
            f8 = ops.attn_fp8_quant(qkv, 3 * D, R, S, H)
            ao, lse = ops.attn_fp8_fwd(f8, SCF, save_lse=need_grad, drop=site(i, 0))
            qkv = None                       # the backward reads the e4m3 copies
        else:
            ao, lse = ops.attn_fwd(qkv, qkv[:, D:], qkv[:, 2 * D:], 3 * D, R, S, H, SCF, kvalid=prep.fusion_kvalid, save_lse=need_grad, drop=site(i, 0),
                                   head_dim=self.hdim)
        xo, post = self._fusion_post_fwd(i, ao, M, xf, None, 1, need_grad and self.adt == BF16, site, need_grad)
        return xo, (dict(pruned=False, x=xf, qkv=qkv, f8=f8, ao=ao, lse=lse, **post) if need_grad else None)

    def _fusion_post_fwd(self, i, ao, rows, residual, ldr, row_mult, bits, site, need_grad):
        """Post-attention half of fusion layer ``i`` on ``rows`` rows: out_proj (+ residual, dropout) -> norm1 -> linear1 (ReLU, dropout) -> linear2 (+ residual, dropout) -> norm2.
        ``ldr``: leading dimension of ``residual`` (position-0 rows of all tokens: S * D); ``row_mult``: row step of the dropout counters; ``bits``: keep linear1's ReLU derivative as bits"""
        D, F, w, l = self.D, self.dff, self._w, self.visual_encoder.fusion_xformer.layers[i]
        h1 = ops.gemm_nt(ao, w[f"f{i}.out"], rows, D, D, bias=l.self_attn.out_proj.bias, residual=residual, ldr=ldr, drop=site(i, 1, row_mult))
        x1, m1, r1 = ops.norm_fwd(h1, l.norm1.weight, l.norm1.bias, 1e-5, rows, save_stats=need_grad, D=D)
        f1b = torch.empty(ops.relu_bits_bytes(rows, F), device=x1.device, dtype=torch.uint8) if bits else None
        f1 = ops.gemm_nt(x1, w[f"f{i}.l1"], rows, F, D, bias=l.linear1.bias, act=ops.ACT_RELU, relu_bits_out=f1b, drop=site(i, 2, row_mult))
        h2 = ops.gemm_nt(f1, w[f"f{i}.l2"], rows, D, F, bias=l.linear2.bias, residual=x1, drop=site(i, 3, row_mult))
        xo, m2, r2 = ops.norm_fwd(h2, l.norm2.weight, l.norm2.bias, 1e-5, rows, save_stats=need_grad, D=D)
        return xo, dict(h1=h1, x1=x1, n1=(m1, r1), f1=f1, f1b=f1b, h2=h2, n2=(m2, r2))

    def _decoder_step_fwd(self, xd, prep):
        """The llama decoder as one KV-cached step: env b attends to cache slots >= max(counter - time_step_b, 0), its current episode (allenact_dino_transformer.py:388-397).
        With ``prep.row_pos`` / ``row_klen`` (/ ``row_cache``): every row on a KV ring of its own instead (ops.kv_append_rows, ops.attn_decode_rows)."""
        D, HD, B, w, SCD = self.D, self.dec_hidden, xd.shape[0], self._w, self.hdim_dec ** -0.5      # B: prep.B, or the leading rows of a vector step
        if self.hdim_dec != 64:
            raise NotImplementedError("KV-cached single steps need 64-wide decoder heads (MFMA / decode attention kernels)")
        t, t_dev = self.time_step_counter, self._t_dev
        per_row = prep.row_pos is not None
        if not per_row:
            self._ensure_caches(B)
        if per_row:
            # per-row KV rings (a vector of episodes with ages of their own): slot, length and cache row of every row come from device memory; the caller has
            # allocated the caches (``_ensure_caches(row_cache.max() + 1)``), and the step counter is neither read nor advanced
            if self._kv is None:
                raise ValueError("row_pos: allocate the KV caches with _ensure_caches(n) before the first per-row step")
        elif t_dev is None:
            start = torch.clamp(t - prep.time_step, min=0)
            kvalid = (torch.arange(t + 1, device=self.device_)[None, :] >= start[:, None]).to(torch.uint8).contiguous()
            S_att = t + 1
        else:
            # captured / recorded form: the step counter lives in device memory, so every kernel argument is step-independent --
            # attention runs over the whole cache window and the mask hides the slots beyond the counter
            kvalid = prep.kvalid_static        # shared by the three towers (a function of the step and time_step only)
            if kvalid is None:
                ar = self._ar_steps
                kvalid = ((ar[None, :] <= t_dev) & (ar[None, :] >= torch.clamp(t_dev - prep.time_step, min=0)[:, None])).to(torch.uint8).contiguous()
            S_att = self.max_steps
        # bf16 product path: RMSNorm folded into the following GEMM (one launch instead of two).  The update's sequence form runs norm -> bf16 -> GEMM (its backward
        # needs the normed activation), so a rollout's old log-probs and the update's recomputed ones differ by that one rounding of the decoder's normed rows --
        # bounded by tests/test_model_gpu.py::test_fused_rmsnorm_step_close_to_unfused; ``rms_fused = False`` runs the acting step on the two-launch form
        fused = self.adt == BF16 and self.rms_fused
        if fused:
            self.refresh_folded()

        def normed_gemm(x, norm, key, n):
            if fused:
                return ops.gemm_nt_rmsa(x, self._wg[key], B, n, D, 1e-5)
            y, _, _ = ops.norm_fwd(x, norm.weight, None, 1e-5, B, rms=True, save_stats=False, D=D)
            return ops.gemm_nt(y, w[key], B, n, D)
        for i, l in enumerate(self.decoder.layers):
            qkv = normed_gemm(xd, l.attention_norm, f"d{i}.qkv", 3 * D)
            cache = self._kv[i]
            cv = cache.view(-1, 2 * D)
            if per_row:
                ops.kv_append_rows(qkv[:, D:], 3 * D, cache, prep.row_cache, prep.row_pos, B, 2 * D)
                ao, _ = ops.attn_decode_rows(qkv, 3 * D, cv, cv[:, D:], 2 * D, prep.row_klen, prep.row_cache, B, self.Hdec, SCD, self.max_steps)
            else:
                if t_dev is None:
                    cache[:B, t].copy_(qkv[:, D:])
                elif self.adt == BF16:
                    ops.kv_append(qkv[:, D:], 3 * D, cache, t_dev, B, 2 * D)
                else:
                    cache[:B].index_copy_(1, t_dev.view(1), qkv[:, D:].unsqueeze(1))
                ao, _ = ops.attn_fwd(qkv, cv, cv[:, D:], 2 * D, B, S_att, self.Hdec, SCD, kvalid=kvalid, save_lse=False, Sq=1, ldq=3 * D,
                                     kv_rows=self.max_steps)
            h = ops.gemm_nt(ao, w[f"d{i}.wo"], B, D, D, residual=xd)
            gg = ops.swiglu_fwd(normed_gemm(h, l.ffn_norm, f"d{i}.w13", 2 * HD), B, HD)
            xd = ops.gemm_nt(gg, w[f"d{i}.w2"], B, D, HD, residual=h)
        if not per_row:
            self.time_step_counter += 1
        return xd

    def _decoder_rows_fwd(self, xd, prep):
        """The acting step of a vector of episodes (``prep.row_pos`` ...): the first B - row_slide rows take the KV-cached step on their rings; the trailing
        ``row_slide`` rows are episodes older than their window of ``row_window`` steps and are decoded over that window (``_decoder_window_fwd``).  With a window
        given, every row's decoder input goes into its history ring first (slot row_pos of history row row_cache; ``_ensure_history``)."""
        B, D, ns = prep.B, self.D, int(prep.row_slide or 0)
        if self.hdim_dec != 64:
            raise NotImplementedError("KV-cached single steps need 64-wide decoder heads (MFMA / decode attention kernels)")
        if self.adt != BF16:
            raise NotImplementedError("the acting step on per-row KV rings exists on the bf16 product path only")
        if prep.row_window:
            if self._hist is None or prep.row_cache is None:
                raise ValueError("row_window: allocate the history with _ensure_history(n, window) and give row_cache")
            ops.kv_append_rows(xd, D, self._hist, prep.row_cache, prep.row_pos, B, D)
        elif ns:
            raise ValueError("row_slide needs row_window")
        outs = ([self._decoder_step_fwd(xd[:B - ns], prep)] if ns < B else []) + ([self._decoder_window_fwd(prep, B - ns, ns)] if ns else [])
        return outs[0] if len(outs) == 1 else torch.cat(outs)

    def _decoder_window_fwd(self, prep, first, n):
        """Rows first ... first + n of a vector step whose episodes have outlived their window W = ``prep.row_window``: the reference's agent decodes the last W
        embedded steps anew (early_fusion_tsfm_models.py:491-497: decoder_input[:, -max_seq_len:]) -- cached K / V of the layers above the first would carry steps
        older than the window in their context.  The window is read from the history ring, oldest step first, and runs through the sequence form of the decoder;
        its causal attention is, for W <= 512, ops.attn_decode_rows with one query row per (episode, position): position t reads the t + 1 first keys of its
        episode.  Above 512 steps (where the tile kernels of the sequence form end) it is the streaming causal kernel of ops.attn_causal_fwd on n rows of W tokens,
        which reads K and V once per 64-query tile instead of once per query; ``WINDOW_DECODE_ROWS`` keeps the single-query rows there too (A/B, tests).
        -> the rows of the newest position [n, D]"""
        W, D, dev = int(prep.row_window), self.D, self.device_
        ar = torch.arange(W, device=dev)
        slot = (prep.row_pos[first:first + n].long()[:, None] + 1 + ar[None, :]) % W                      # oldest ... newest (= row_pos, just written)
        xw = self._hist[prep.row_cache[first:first + n].long()[:, None], slot].reshape(n * W, D)      # rows (b * W + t)
        pw = Prep()
        pw.T, pw.B, pw.R = W, n, n * W
        if W > MAX_TILE_SEQ and not WINDOW_DECODE_ROWS:
            pw.traj_bt = None                                                                         # one episode per row: plain causal
            xo, _ = self._decoder_seq_fwd(xw, pw, False)
        else:
            xo, _ = self._decoder_seq_fwd(xw, pw, False, attn=self._window_rows_attn(n, W))
        return xo.view(n, W, D)[:, W - 1].contiguous()

    def _window_rows_attn(self, n, W):
        """Causal attention over n sequences of W steps as a callable qkv -> (ao, lse) on ops.attn_decode_rows: one single-query row per (sequence, position),
        position t reading the t + 1 first keys of its sequence (any W <= 1024)"""
        D, dev = self.D, self.device_
        crow = torch.arange(n, device=dev, dtype=torch.int32).repeat_interleave(W)
        klen = (torch.arange(W, device=dev) + 1).to(torch.int32).repeat(n)
        return lambda qkv: ops.attn_decode_rows(qkv, 3 * D, qkv[:, D:], qkv[:, 2 * D:], 3 * D, klen, crow, n * W, self.Hdec, self.hdim_dec ** -0.5, W)

    def _check_seq_len(self, T, need_grad):
        """Sequences above MAX_TILE_SEQ steps run forward only, on the bf16 path with 64-wide decoder heads (csrc/attn_seq_long.hip); refused before any launch"""
        if T <= MAX_TILE_SEQ:
            return
        if need_grad:
            raise ValueError(f"T = {T}: the attention backward ends at {MAX_TILE_SEQ} steps; longer sequences are forward only (torch.no_grad() or eval mode)")
        if self.adt != BF16:
            raise ValueError(f"T = {T}: the fp32 verification mode ends at {MAX_TILE_SEQ} steps (the causal forward above that exists in bf16 only)")
        if self.hdim_dec != 64:
            raise ValueError(f"T = {T}: decoder heads of {self.hdim_dec} end at {MAX_TILE_SEQ} steps (the causal forward above that is built for 64-wide heads)")
        if T > MAX_ACTING_WINDOW:
            raise ValueError(f"T = {T}: the causal forward is limited to {MAX_ACTING_WINDOW} steps")

    def _decoder_seq_fwd(self, xd, prep, need_grad, attn=None):
        """The llama decoder over whole sequences, rows (b*T + t), causal within a trajectory -> (output rows, saved activations per layer).  T <= 512: the block-causal
        tile kernels.  512 < T <= 1024, forward only: the streaming causal kernel (ops.attn_causal_fwd; ``prep.traj_bt`` None: one trajectory per row).
        ``attn``: the causal attention as a callable qkv -> (ao, lse) instead (forward only: ``_decoder_window_fwd``)"""
        D, HD, T, B, R, w, SCD = self.D, self.dec_hidden, prep.T, prep.B, prep.R, self._w, self.hdim_dec ** -0.5
        if attn is None:
            self._check_seq_len(T, need_grad)
        dl = []
        for i, l in enumerate(self.decoder.layers):
            n1, _, r1 = ops.norm_fwd(xd, l.attention_norm.weight, None, 1e-5, R, rms=True, save_stats=need_grad, D=D)
            qkv = ops.gemm_nt(n1, w[f"d{i}.qkv"], R, 3 * D, D)
            if attn is not None:
                ao, lse = attn(qkv)
            elif T > MAX_TILE_SEQ:
                ao, lse = ops.attn_causal_fwd(qkv, qkv[:, D:], qkv[:, 2 * D:], 3 * D, B, T, self.Hdec, SCD, traj=prep.traj_bt)
            else:
                ao, lse = ops.attn_fwd(qkv, qkv[:, D:], qkv[:, 2 * D:], 3 * D, B, T, self.Hdec, SCD, head_dim=self.hdim_dec, mask_mode=ops.MASK_BLOCK_CAUSAL,
                                       traj=prep.traj_bt, save_lse=need_grad)
            h = ops.gemm_nt(ao, w[f"d{i}.wo"], R, D, D, residual=xd)
            n2, _, r2 = ops.norm_fwd(h, l.ffn_norm.weight, None, 1e-5, R, rms=True, save_stats=need_grad, D=D)
            ab = ops.gemm_nt(n2, w[f"d{i}.w13"], R, 2 * HD, D)
            gg = ops.swiglu_fwd(ab, R, HD)
            xo = ops.gemm_nt(gg, w[f"d{i}.w2"], R, D, HD, residual=h)
            if need_grad:
                dl.append(dict(x=xd, n1=n1, r1=r1, qkv=qkv, ao=ao, lse=lse, h=h, n2=n2, r2=r2, ab=ab, g=gg))
            xd = xo
        return xd, dl

    def _heads_fwd(self, xd, prep, c, need_grad):
        """final RMSNorm + output projection -> beliefs (fp32, rows b*T + t) -> actor logits and critic values (rows t*B + b)"""
        D, T, B, R = self.D, prep.T, prep.B, prep.R
        nf, _, rf = ops.norm_fwd(xd, self.decoder.norm.weight, None, 1e-5, R, rms=True, save_stats=need_grad, D=D)
        beliefs = ops.gemm_nt(nf, self._w["dout"], R, D, D, out_f32=True)
        logits = ops.small_linear_fwd(beliefs, self.actor.linear.weight, self.actor.linear.bias, T, B)
        self._last_full_logits = None        # [T, B, 101] fp32 (critic_type == "discrete"), read by the 3-tower wrapper / engine
        if self.critic_type == "linear":
            values = ops.small_linear_fwd(beliefs, self.critic.fc.weight, self.critic.fc.bias, T, B)
        else:
            values, self._last_full_logits, c["head"] = self._critic_head_fwd(beliefs, T, B)
        c.update(xd_last=xd, nf=nf, rf=rf, beliefs=beliefs)
        return logits, values

    # ---- MLP / discrete critic heads (fp32, strided-GEMM kernel; rows come in decoder order b*T + t, leave in (t*B + b)) --------
    def _critic_head_fwd(self, beliefs, T, B):
        R, dims, fc = T * B, self._head_dims, self.critic.fc
        hs = [beliefs]
        for j in range(len(dims) - 1):
            last = j == len(dims) - 2
            hs.append(ops.gemm_f32(hs[-1], fc[2 * j].weight, R, dims[j + 1], dims[j], bias=fc[2 * j].bias, act=ops.ACT_NONE if last else ops.ACT_RELU))
        out_tb = hs[-1].view(B, T, dims[-1]).transpose(0, 1).contiguous()           # -> rows (t*B + b)
        if self.critic_type == "discrete":
            values, _, _ = ops.hlgauss_fwd_bwd(out_tb.view(R, dims[-1]), None, None, self.critic.loss_fn.min_value, self.critic.loss_fn.max_value,
                                               self.critic.loss_fn.sigma, want_grad=False)
            return values, out_tb, hs
        return out_tb.reshape(R), None, hs

    def _critic_head_bwd(self, hs, T, B, dvalues, dfull, dbel, accumulate_dx):
        """dvalues [T,B,1] and/or dfull [T,B,101] -> parameter grads (arena) and dbel [R,512] (rows b*T + t)."""
        R, dims, fc, g = T * B, self._head_dims, self.critic.fc, self.g
        if self.critic_type == "discrete":
            lf = self.critic.loss_fn
            flog_tb = hs[-1].view(B, T, dims[-1]).transpose(0, 1).contiguous().view(R, dims[-1])
            d_tb = None
            if dvalues is not None:      # gradient through the read-out value = sum softmax * centres
                _, d_tb, _ = ops.hlgauss_fwd_bwd(flog_tb, None, dvalues.reshape(R).contiguous(), lf.min_value, lf.max_value, lf.sigma, want_values=False)
            if dfull is not None:
                d_tb = dfull.reshape(R, dims[-1]) if d_tb is None else d_tb + dfull.reshape(R, dims[-1])
        else:
            d_tb = dvalues.reshape(R, 1)
        dy = d_tb.view(T, B, dims[-1]).transpose(0, 1).contiguous().view(R, dims[-1]).float()     # back to decoder order
        for j in reversed(range(len(dims) - 1)):
            n_out, n_in, x = dims[j + 1], dims[j], hs[j]
            w = fc[2 * j].weight
            ops.gemm_f32(dy, x, n_out, n_in, R, sa=(1, n_out), sb=(1, n_in), out=g(w), accumulate=True)      # dW += dY^T X
            ops.colsum_f32(dy, g(fc[2 * j].bias), R, n_out)
            if j == 0:
                ops.gemm_f32(dy, w, R, n_in, n_out, sb=(1, n_in), out=dbel, accumulate=accumulate_dx)       # dX = dY W
            else:
                dy = ops.gemm_f32(dy, w, R, n_in, n_out, sb=(1, n_in), mask=x)                              # ... through the ReLU

    # ---- backward: the same stages in reverse ----------------------------------------------------------------------------------
    def run_backward(self, prep: "Prep", c, dlogits: Optional[torch.Tensor], dvalues: Optional[torch.Tensor],
                     dfull_logits: Optional[torch.Tensor] = None):
        """Accumulates parameter gradients into the arena's flat grad buffer.  ``dfull_logits``: gradient of the discrete critic's
        bin logits (HL-Gauss loss), critic_type == "discrete" only."""
        D, T, B, R, S, g = self.D, prep.T, prep.B, prep.R, prep.S, self.g
        Rf, ragged = prep.Rf, prep.row_map is not None
        dx = self._heads_bwd(prep, c, dlogits, dvalues, dfull_logits)
        if dx is None:
            return
        dx = self._decoder_seq_bwd(prep, c, dx)
        # gradient of the fusion transformer's output: the position-0 rows only behind a pruned last layer, else all token rows (zero but for position 0)
        pruned = bool(c["fusion"]) and c["fusion"][-1]["pruned"]
        dyf = torch.empty(Rf, D, device=self.device_, dtype=self.adt) if pruned else ops.zeros(Rf, S, D, device=self.device_, dtype=self.adt).view(Rf * S, D)
        ldy = D if pruned else S * D
        # compact fusion rows: the kernel leaves the decoder-input gradient in decoder-row order (the embedding tables take every row's, a padded step's is zero), and
        # the inverse table brings the valid steps' rows back -- a gather, the map being injective
        dyr = torch.empty(R, D, device=self.device_, dtype=self.adt) if ragged else dyf
        ops.decoder_embed_bwd(dx, prep.prev_actions if self.has_prev else None, prep.masks if self.has_prev else None, prep.hand if self.has_hand else None, T, B,
                              dyr, D if ragged else ldy, g(self.last_actions_embed.weight) if self.has_prev else None,
                              g(self.object_in_hand_embed.weight) if self.has_hand else None)
        if ragged:
            es = dyr.element_size()
            ops.rows_gather(dyf, ldy * es, dyr, D * es, prep.row_inv, Rf, D * es, R)
        site = self._site_fn(c.get("drop_seed"))
        drop_scale = 1.0 / (1.0 - self.dropout_p) if c.get("drop_seed") is not None else 1.0
        for i in reversed(range(len(c["fusion"]))):
            dyf = self._fusion_layer_bwd(i, c["fusion"][i], dyf, prep, site, drop_scale)
            c["fusion"][i] = None        # the layer's saved activations go before the next layer allocates
        self._inputs_bwd(prep, c, dyf)

    def _heads_bwd(self, prep, c, dlogits, dvalues, dfull_logits):
        """actor / critic heads, output projection and final RMSNorm -> the gradient of the decoder's output rows (None: no head received a gradient)"""
        D, T, B, R, g = self.D, prep.T, prep.B, prep.R, self.g
        dbel = torch.empty(R, D, device=self.device_, dtype=F32)
        acc = False      # the first head that has a gradient writes dbel, the next one adds to it
        for head, dy in ((self.actor.linear, dlogits),) + (((self.critic.fc, dvalues),) if self.critic_type == "linear" else ()):
            if dy is not None:
                ops.small_linear_bwd(c["beliefs"], head.weight, dy.reshape(R, -1).contiguous(), dbel, g(head.weight), g(head.bias), T, B, accumulate_dx=acc)
                acc = True
        if self.critic_type != "linear" and (dvalues is not None or dfull_logits is not None):
            self._critic_head_bwd(c["head"], T, B, dvalues, dfull_logits, dbel, accumulate_dx=acc)
            acc = True
        if not acc:
            return None
        dy = torch.empty(R, D, device=self.device_, dtype=self.adt)
        ops.cast_bf16(dbel, dy)
        ops.gemm_tn_acc(dy, c["nf"], self._dw["dout"], R, D, D)
        dnf = ops.gemm_nt(dy, self._wt["dout"], R, D, D)
        return ops.norm_bwd(dnf, c["xd_last"], self.decoder.norm.weight, None, None, c["rf"], R, g(self.decoder.norm.weight), None, rms=True, D=D)

    def _decoder_seq_bwd(self, prep, c, dx):
        """backward of ``_decoder_seq_fwd``: gradient of the decoder's output rows -> gradient of its input rows"""
        D, HD, T, B, R, wt, dw, g, SCD = self.D, self.dec_hidden, prep.T, prep.B, prep.R, self._wt, self._dw, self.g, self.hdim_dec ** -0.5
        for i in reversed(range(len(self.decoder.layers))):
            l, a = self.decoder.layers[i], c["dec"][i]
            ops.gemm_tn_acc(dx, a["g"], dw[f"d{i}.w2"], R, D, HD)
            dg = ops.gemm_nt(dx, wt[f"d{i}.w2"], R, HD, D)
            dab = ops.swiglu_bwd(a["ab"], dg, R, HD)
            ops.gemm_tn_acc(dab, a["n2"], dw[f"d{i}.w13"], R, 2 * HD, D)
            dn2 = ops.gemm_nt(dab, wt[f"d{i}.w13"], R, D, 2 * HD)
            dh = ops.norm_bwd(dn2, a["h"], l.ffn_norm.weight, None, None, a["r2"], R, g(l.ffn_norm.weight), None, rms=True, dres=dx, D=D)
            ops.gemm_tn_acc(dh, a["ao"], dw[f"d{i}.wo"], R, D, D)
            dao = ops.gemm_nt(dh, wt[f"d{i}.wo"], R, D, D)
            dqkv = torch.empty(R, 3 * D, device=self.device_, dtype=self.adt)
            q = a["qkv"]
            ops.attn_bwd(q, q[:, D:], q[:, 2 * D:], 3 * D, a["ao"], D, a["lse"], dao, D, dqkv, dqkv[:, D:], dqkv[:, 2 * D:], 3 * D,
                         B, T, self.Hdec, SCD, mask_mode=ops.MASK_BLOCK_CAUSAL, traj=prep.traj_bt, head_dim=self.hdim_dec)
            ops.gemm_tn_acc(dqkv, a["n1"], dw[f"d{i}.qkv"], R, 3 * D, D)
            dn1 = ops.gemm_nt(dqkv, wt[f"d{i}.qkv"], R, D, 3 * D)
            dx = ops.norm_bwd(dn1, a["x"], l.attention_norm.weight, None, None, a["r1"], R, g(l.attention_norm.weight), None, rms=True, dres=dh, D=D)
        return dx

    @staticmethod
    def _relu_bwd_gemm(dy, wt, rows, n, k, act, bits, alpha=1.0):
        """alpha * (dy @ wt^T) where the forward's ReLU output ``act`` was positive: by its sign ``bits`` if the forward kept them, else by the stored activation (fp32 mode, pruned rows)"""
        return ops.gemm_nt(dy, wt, rows, n, k, alpha=alpha, **(dict(relu_bits=bits) if bits is not None else dict(relu_mask=act)))

    def _fusion_post_bwd(self, i, a, dyf, rows, row_mult, site, drop_scale):
        """backward of ``_fusion_post_fwd``: gradient of the layer's output rows -> (dao, dh1), the gradients of the attention output and of the residual path into its input"""
        D, F, wt, dw, g, l = self.D, self.dff, self._wt, self._dw, self.g, self.visual_encoder.fusion_xformer.layers[i]
        d3, d1 = site(i, 3, row_mult), site(i, 1, row_mult)
        df = torch.empty_like(a["h2"]) if d3 is not None else None      # under dropout norm_bwd has a second output: the gradient of the dropped-out sub-layer output
        dh2 = ops.norm_bwd(dyf, a["h2"], l.norm2.weight, l.norm2.bias, a["n2"][0], a["n2"][1], rows, g(l.norm2.weight), g(l.norm2.bias),
                           dx_drop=df, drop=d3, D=D)
        df = dh2 if df is None else df               # grad of linear2's output (through dropout2); dh2 = residual-path grad
        ops.gemm_tn_acc(df, a["f1"], dw[f"f{i}.l2"], rows, D, F, db=g(l.linear2.bias))
        # f1 and its sign bits were taken after ReLU and dropout: positive <=> (pre-activation > 0 and kept); alpha = the dropout scale
        df1 = self._relu_bwd_gemm(df, wt[f"f{i}.l2"], rows, F, D, a["f1"], a["f1b"], alpha=drop_scale)
        ops.gemm_tn_acc(df1, a["x1"], dw[f"f{i}.l1"], rows, F, D, db=g(l.linear1.bias))
        dx1 = ops.gemm_nt(df1, wt[f"f{i}.l1"], rows, D, F, residual=dh2)
        del df1, df                                  # [rows, dff]: freed before the next allocation
        da = torch.empty_like(a["h1"]) if d1 is not None else None
        dh1 = ops.norm_bwd(dx1, a["h1"], l.norm1.weight, l.norm1.bias, a["n1"][0], a["n1"][1], rows, g(l.norm1.weight), g(l.norm1.bias),
                           dx_drop=da, drop=d1, D=D)
        da = dh1 if da is None else da
        ops.gemm_tn_acc(da, a["ao"], dw[f"f{i}.out"], rows, D, D, db=g(l.self_attn.out_proj.bias))
        return ops.gemm_nt(da, wt[f"f{i}.out"], rows, D, D), dh1

    def _fusion_layer_bwd(self, i, a, dyf, prep, site, drop_scale):
        """Backward of fusion layer ``i``: the gradient of its output rows -> the gradient of its input rows [R * S, D]"""
        D, H, R, S, w, wt, dw, g, SCF = self.D, self.H, prep.Rf, prep.S, self._w, self._wt, self._dw, self.g, self.hdim ** -0.5      # R: fusion rows
        M, l = R * S, self.visual_encoder.fusion_xformer.layers[i]
        if a["pruned"]:
            dao, dh1 = self._fusion_post_bwd(i, a, dyf, R, S, site, drop_scale)
            gb = g(l.self_attn.in_proj_bias)
            if a["absorbed"]:
                # backward of the absorbed form (_fusion_layer_fwd): dc_h = W_v,h^T do_h, dsigma_h = do_h . b_v,h; the streaming kernel returns dX of every token
                # and dqt; every weight gradient goes through the accumulating GEMM / column sum (deterministic mode included).  The K third of the bias
                # gradient is exactly zero (sum_j dS_hj = 0) and is not touched.
                w_in, wt_in, dw_in = w[f"f{i}.in"], wt[f"f{i}.in"], dw[f"f{i}.in"]
                edao, dsig, sdao = ops.head_expand(dao, R, bias=l.self_attn.in_proj_bias[2 * D:], sigma=a["sig"])
                dcc = ops.gemm_nt(edao, wt_in[:, 2 * D:], 8 * R, D, D)
                ops.gemm_tn_acc(edao, a["cc"], dw_in[2 * D:], 8 * R, D, D)                   # dW_v,h += do_h c_h^T
                ops.colsum_acc(sdao, gb[2 * D:], R, D)                                       # db_v,h += sigma_h do_h
                dx, dqt = ops.attn_q1_bwd(a["x"], S * D, a["qt"], dcc, dsig, a["prob"], R, S, SCF, drop=site(i, 0))
                dx = dx.view(M, D)
                ops.gemm_tn_acc(a["eq"], dqt, dw_in[D:2 * D], 8 * R, D, D)                   # dW_k,h += q_h dqt_h^T
                dq0 = ops.head_pick(ops.gemm_nt(dqt, w_in[D:2 * D], 8 * R, D, D), R)         # W_k,h dqt_h
                ops.gemm_tn_acc(dq0, a["x"], dw_in[:D], R, D, D, ldx=S * D, db=gb[:D])
            else:
                dq0 = torch.empty(R, D, device=self.device_, dtype=self.adt)
                dkv = torch.empty(M, 2 * D, device=self.device_, dtype=self.adt)
                kv = a["kv"]
                ops.attn_bwd(a["q0"], kv, kv[:, D:], 2 * D, a["ao"], D, a["lse"], dao, D, dq0, dkv, dkv[:, D:], 2 * D, R, S, H, SCF, head_dim=self.hdim,
                             Sq=1, ldq=D, lddq=D, drop=site(i, 0))
                ops.gemm_tn_acc(dkv, a["x"], dw[f"f{i}.in"][D:], M, 2 * D, D, db=gb[D:])
                ops.gemm_tn_acc(dq0, a["x"], dw[f"f{i}.in"][:D], R, D, D, ldx=S * D, db=gb[:D])
                dx = ops.gemm_nt(dkv, wt[f"f{i}.in"][:, D:], M, D, 2 * D)                    # dX through K and V, all tokens
            t0 = ops.gemm_nt(dq0, wt[f"f{i}.in"][:, :D], R, D, D, residual=dh1)             # position 0: Q path + residual path
            ops.rows_add(dx, S * D, t0, D, R, D)
            return dx
        dao, dh1 = self._fusion_post_bwd(i, a, dyf, M, 1, site, drop_scale)
        dqkv = torch.empty(M, 3 * D, device=self.device_, dtype=self.adt)
        q = a["qkv"]
        if a["f8"] is not None:
            ops.attn_fp8_bwd(a["f8"], a["ao"], a["lse"], dao, dqkv, dqkv[:, D:], dqkv[:, 2 * D:], 3 * D, SCF, drop=site(i, 0))
        else:
            ops.attn_bwd(q, q[:, D:], q[:, 2 * D:], 3 * D, a["ao"], D, a["lse"], dao, D, dqkv, dqkv[:, D:], dqkv[:, 2 * D:], 3 * D,
                         R, S, H, SCF, drop=site(i, 0), head_dim=self.hdim)
        ops.gemm_tn_acc(dqkv, a["x"], dw[f"f{i}.in"], M, 3 * D, D, db=g(l.self_attn.in_proj_bias))
        return ops.gemm_nt(dqkv, wt[f"f{i}.in"], M, D, 3 * D, residual=dh1)

    def _inputs_bwd(self, prep, c, dx0):
        """backward of ``_inputs_fwd``: gradient of the fusion transformer's input rows -> fusion token, text adapter (frozen text encoder), visual adapter + compressor"""
        D, T, B, R, S, L, U = self.D, prep.T, prep.B, prep.Rf, prep.S, prep.L, prep.U      # R: fusion rows
        ve, wt, dw, g, dev = self.visual_encoder, self._wt, self._dw, self.g, self.device_
        M2 = R * self.ncam * NPATCH
        ops.colsum_acc(dx0, g(ve.fusion_token), R, D, row_stride=S)
        # text adapter (trainable) -- the T5 encoder is frozen (no_grad in the reference)
        dtf = ops.zeros(U * L, D, device=dev, dtype=F32)
        if prep.row_seg is not None:
            # compact rows lie goal by goal: the segmented form, one wave per (goal, token) over that goal's rows, plain stores (repeatable without a shadow)
            ops.fusion_text_bwd_seg(dx0, prep.row_seg, U, S, L, self.text_off, dtf)
        elif ops.det_active():       # deterministic mode: this accumulated intermediate gets its own fixed-point shadow (slot 1)
            dtf_sh = torch.zeros(U * L * D, device=dev, dtype=torch.int64)
            ops.det_config(1, dtf, dtf_sh)
            try:
                ops.fusion_text_bwd(dx0, prep.gid, T, B, S, L, self.text_off, dtf)
                ops.det_finalize(dtf, dtf_sh)
            finally:
                ops.det_config(1, None, None)
        else:
            ops.fusion_text_bwd(dx0, prep.gid, T, B, S, L, self.text_off, dtf)
        dtf_b = torch.empty(U * L, D, device=dev, dtype=self.adt)
        ops.cast_bf16(dtf, dtf_b)
        dta = ops.norm_bwd(dtf_b, c["ta"], ve.text_adapter[1].weight, ve.text_adapter[1].bias, c["ta_stats"][0], c["ta_stats"][1], U * L,
                           g(ve.text_adapter[1].weight), g(ve.text_adapter[1].bias), relu=True, D=D)
        ops.gemm_tn_acc(dta, c["t5"], dw["ta"], U * L, D, self.text_dim, db=g(ve.text_adapter[0].bias))
        # visual adapter + compressor (all cameras in one batch)
        da1 = ops.norm_bwd(dx0, c["a1"], ve.visual_adapter[1].weight, ve.visual_adapter[1].bias, c["va"][0], c["va"][1], M2,
                           g(ve.visual_adapter[1].weight), g(ve.visual_adapter[1].bias), relu=True, dtok=self._dcamtok,
                           tok_group=NPATCH, dymap=(self.ncam * NPATCH, S, 1), D=D)
        ops.gemm_tn_acc(da1, c["c2"], dw["va"], M2, D, D, db=g(ve.visual_adapter[0].bias))
        dc2 = self._relu_bwd_gemm(da1, wt["va"], M2, D, D, c["c2"], c["c2b"])
        ops.gemm_tn_acc(dc2, c["c1"], dw["c2"], M2, D, D, db=g(ve.visual_compressor[2].bias))
        dc1 = self._relu_bwd_gemm(dc2, wt["c2"], M2, D, D, c["c1"], c["c1b"])
        ops.gemm_tn_acc(dc1, prep.tokens.view(M2, self.dino_dim), dw["c1"], M2, D, self.dino_dim, db=g(ve.visual_compressor[0].bias))


# ================================================================================================ frozen T5
class T5Frozen(nn.Module):
    """Frozen HF ``T5EncoderModel('t5-small')`` geometry (allenact_dino_transformer.py:506-508,599-603); state_dict
    names equal HF's.  Runs on the same bf16 GEMM / attention / RMS-norm kernels, once per unique goal."""

    def __init__(self, device, vocab=32128, d=512, h=8, dff=2048, n_layers=6, buckets=32, max_distance=128):
        super().__init__()
        self.device_ = device
        self.h, self.dff, self.buckets, self.max_distance = h, dff, buckets, max_distance

        def P(*shape, scale=None):
            t = torch.randn(*shape) * (scale if scale is not None else 1.0 / math.sqrt(shape[-1]))
            return nn.Parameter(t.to(device), requires_grad=False)

        self.shared = _NS(); self.shared.weight = P(vocab, d, scale=1.0)
        self.encoder = _NS()
        self.encoder.embed_tokens = _NS(); self.encoder.embed_tokens.weight = self.shared.weight   # tied, as in HF
        self.encoder.block = nn.ModuleList()
        for i in range(n_layers):
            b = _NS(); b.layer = nn.ModuleList([_NS(), _NS()])
            sa = b.layer[0].SelfAttention = _NS()
            for n in ("q", "k", "v", "o"):
                setattr(sa, n, _NS()); getattr(sa, n).weight = P(d, d)
            if i == 0:
                sa.relative_attention_bias = _NS(); sa.relative_attention_bias.weight = P(buckets, h, scale=0.5)
            b.layer[0].layer_norm = _NS(); b.layer[0].layer_norm.weight = nn.Parameter(torch.ones(d, device=device), requires_grad=False)
            ff = b.layer[1].DenseReluDense = _NS()
            ff.wi = _NS(); ff.wi.weight = P(dff, d)
            ff.wo = _NS(); ff.wo.weight = P(d, dff)
            b.layer[1].layer_norm = _NS(); b.layer[1].layer_norm.weight = nn.Parameter(torch.ones(d, device=device), requires_grad=False)
            self.encoder.block.append(b)
        self.encoder.final_layer_norm = _NS()
        self.encoder.final_layer_norm.weight = nn.Parameter(torch.ones(d, device=device), requires_grad=False)
        self._rt = self._rt_dtype = None
        self._bias_cache: Dict[int, torch.Tensor] = {}

    def sync(self, dtype=BF16):
        """(re)build the runtime copies (bf16, or fp32 in the verification mode) of the frozen weights."""
        rt = []
        for b in self.encoder.block:
            sa, ff = b.layer[0].SelfAttention, b.layer[1].DenseReluDense
            qkv32 = torch.cat([sa.q.weight, sa.k.weight, sa.v.weight], 0).float()
            g0, g1 = b.layer[0].layer_norm.weight.float(), b.layer[1].layer_norm.weight.float()
            rt.append(dict(qkv=qkv32.to(dtype).contiguous(),
                           o=sa.o.weight.to(dtype).contiguous(), wi=ff.wi.weight.to(dtype).contiguous(),
                           wo=ff.wo.weight.to(dtype).contiguous(),
                           # T5LayerNorm folded into the following linear for the norm-fused small-M GEMMs (ops.gemm_nt_rmsa): W * gamma[None, :]
                           qkv_g=(qkv32 * g0[None, :]).to(dtype).contiguous(), wi_g=(ff.wi.weight.float() * g1[None, :]).to(dtype).contiguous()))
        self._rt, self._rt_dtype = rt, dtype
        self._bias_cache.clear()

    def position_bias(self, L: int) -> torch.Tensor:
        if L not in self._bias_cache:
            pos = torch.arange(L, device=self.device_)
            rel = pos[None, :] - pos[:, None]
            nb = self.buckets // 2
            out = (rel > 0).long() * nb
            a = rel.abs()
            max_exact = nb // 2
            big = max_exact + (torch.log(a.float().clamp(min=1) / max_exact) / math.log(self.max_distance / max_exact) * (nb - max_exact)).long()
            big = torch.minimum(big, torch.full_like(big, nb - 1))
            bucket = out + torch.where(a < max_exact, a, big)
            tab = self.encoder.block[0].layer[0].SelfAttention.relative_attention_bias.weight
            self._bias_cache[L] = tab[bucket].permute(2, 0, 1).contiguous().float()
        return self._bias_cache[L]

    T5_STREAM = 64      # dropout stream ids of the text encoder: 62 embedding, 63 final, 64 + 4*block + {0 probs, 1 attn out, 2 ff act, 3 ff out}

    @torch.no_grad()
    def encode(self, ids: torch.Tensor, attn_mask: torch.Tensor, drop_seed: Optional[int] = None, drop_p: float = 0.1, dtype=BF16,
               seed_dev: Optional[torch.Tensor] = None, fused: Optional[bool] = None) -> torch.Tensor:
        """ids, attn_mask [U, L] int64 (device) -> last_hidden_state [U*L, 512] bf16.

        ``drop_seed``: the text encoder is frozen (no_grad) but NOT in eval mode in the reference -- the policy's ``self.train()``
        (allenact_dino_transformer.py:193) switches HF T5's dropout 0.1 on too -- so in train mode its six
        dropout sites per block / stack are applied here as well.  One realisation per unique goal and forward pass (the reference
        re-encodes the goal for every (t, b) row and so draws a fresh mask per row)."""
        if self._rt is None or self._rt_dtype != dtype:
            self.sync(dtype)
        U, L = ids.shape
        n = U * L
        # seed_dev: recorded / captured passes read the pass seed from device memory (fresh noise per replay), like the fusion layers' sites
        site = (lambda k: ops.Dropout(drop_seed, k, drop_p, seed_dev=seed_dev)) if drop_seed is not None and drop_p > 0 else (lambda k: None)
        x = ops.embed_gather(self.shared.weight, ids.reshape(-1).contiguous(), dtype=dtype)
        ops.dropout_(x, site(62))
        bias = self.position_bias(L)
        kvalid = attn_mask if attn_mask.dtype == torch.uint8 else attn_mask.to(torch.uint8).contiguous()   # uint8 given: no torch op (recorded steps)
        # small passes (an acting step's 64 goals x 12 tokens; an update's unique goals): norm + GEMM in one launch.  ``fused`` given: the caller fixes the form --
        # acting and update passes must share ONE arithmetic: with t5_dropout_per_row the update encodes every (t, b) row (n = R L >> 8192, two-launch form),
        # so the wrapper pins the acting steps to the two-launch form as well
        fused = dtype == BF16 and (n <= 8192 if fused is None else bool(fused))
        for i, (b, rt) in enumerate(zip(self.encoder.block, self._rt)):
            s0 = self.T5_STREAM + 4 * i
            if fused:
                qkv = ops.gemm_nt_rmsa(x, rt["qkv_g"], n, 3 * D, D, 1e-6)
            else:
                nrm, _, _ = ops.norm_fwd(x, b.layer[0].layer_norm.weight, None, 1e-6, n, rms=True, save_stats=False)
                qkv = ops.gemm_nt(nrm, rt["qkv"], n, 3 * D, D)
            ao, _ = ops.attn_fwd(qkv, qkv[:, D:], qkv[:, 2 * D:], 3 * D, U, L, self.h, 1.0, bias=bias, kvalid=kvalid, save_lse=False,
                                 drop=site(s0))
            x = ops.gemm_nt(ao, rt["o"], n, D, D, residual=x, drop=site(s0 + 1))
            if fused:
                hdn = ops.gemm_nt_rmsa(x, rt["wi_g"], n, self.dff, D, 1e-6, act=ops.ACT_RELU, drop=site(s0 + 2))
            else:
                nrm, _, _ = ops.norm_fwd(x, b.layer[1].layer_norm.weight, None, 1e-6, n, rms=True, save_stats=False)
                hdn = ops.gemm_nt(nrm, rt["wi"], n, self.dff, D, act=ops.ACT_RELU, drop=site(s0 + 2))
            x = ops.gemm_nt(hdn, rt["wo"], n, D, self.dff, residual=x, drop=site(s0 + 3))
        out, _, _ = ops.norm_fwd(x, self.encoder.final_layer_norm.weight, None, 1e-6, n, rms=True, save_stats=False)
        ops.dropout_(out, site(63))
        return out


# ================================================================================================ shared per-call inputs
class Prep:
    """Per-forward inputs shared by the three towers (built once).  Producers fill the fields one by one; a name that is not declared here is an AttributeError.
    R = T * B rows of S = 1 + ncam * 84 + L fusion tokens; U unique goals of L tokens; tokens [R, ncam, 84, dino_dim]; prev_actions, masks, hand, time_step [R]
    (hand: None without the in-hand sensor; prev_actions, masks: None without the previous-action sensor); traj_bt [B, T]; ids, attn_mask [U, L]; gid [R]: row -> goal.
    Optional: ``acting`` (a T = 1 pass under no_grad is a step against the KV caches), ``ids_key`` (host-side identity of the goals: eval-mode text-feature cache), ``attn_mask_u8`` (attn_mask in the kernels' format), ``kvalid_static`` (recorded steps: the KV-window mask [B, max_steps]).
    ``fusion_kvalid`` (uint8 [R, S]: the fusion tokens of a row that are keys -- hides the padded goal tokens of a batch of goals of different lengths; forward only).
    ``row_pos``, ``row_klen`` (int32 [B], given together) and ``row_cache`` (int32 [B] or None = identity): the acting step on per-row KV rings -- row b writes slot
    row_pos[b] of cache row row_cache[b] and attends to that cache row's first row_klen[b] slots; the tower's own step counter takes no part.  ``row_window`` (int W)
    and ``row_slide`` (int): with a window every row's decoder input is kept in a history ring of W slots, and the trailing row_slide rows -- episodes that have
    outlived W steps -- are decoded anew over their last W steps instead of against the KV ring.
    ``Rf``, ``row_map``, ``row_inv``, ``row_seg`` (given together; the imitation-learning model's batches of unequal-length trajectories): everything in front of the
    decoder runs on Rf <= R "compact" rows -- the valid steps, trajectory by trajectory -- so tokens is [Rf, ...] and gid [Rf]; row_map int32 [R]: decoder row
    (t * B + b) -> its compact row, or -1 for a padded step (which enters the decoder with a zero fusion feature); row_inv int32 [Rf]: the inverse; row_seg int32
    [U + 1]: goal u owns the compact rows row_seg[u] ... row_seg[u + 1].  The decoder-side fields (prev_actions ... time_step, traj_bt) stay [R].  Update passes on the
    bf16 path only.  The RL towers never set them: Rf = R."""
    __slots__ = ("T", "B", "R", "S", "L", "U", "tokens", "prev_actions", "masks", "hand", "time_step", "traj_bt", "ids", "attn_mask", "gid",
                 "acting", "ids_key", "attn_mask_u8", "kvalid_static", "fusion_kvalid", "row_cache", "row_pos", "row_klen", "row_window", "row_slide",
                 "_Rf", "row_map", "row_inv", "row_seg")

    def __init__(self):
        self.acting, self.ids_key, self.attn_mask_u8, self.kvalid_static = True, None, None, None
        self.fusion_kvalid = self.row_cache = self.row_pos = self.row_klen = self.row_window = self.row_slide = None
        self._Rf = self.row_map = self.row_inv = self.row_seg = None

    @property
    def Rf(self):
        """rows in front of the decoder (fusion rows); R unless a producer set fewer (il.EarlyFusionCnnTransformer.prepare with skip_padded_steps)"""
        return self.R if self._Rf is None else self._Rf

    @Rf.setter
    def Rf(self, n):
        self._Rf = n


class _ActingState(Prep):
    """A recorded / captured acting step: the Prep fields are its static input buffers; + device-resident step counter and indices, graph or per-tower plans, outputs, grouped replays"""
    __slots__ = ("t_dev", "ar_steps", "graph", "plans", "outs", "gplans", "grouped_ok")

    def __init__(self):
        super().__init__()
        self.graph, self.plans, self.outs, self.gplans, self.grouped_ok = None, None, None, {}, False


class _TowerFn(torch.autograd.Function):
    """One autograd node per tower: explicit kernel schedules inside, reference-style ``loss.backward()`` outside."""

    @staticmethod
    def forward(ctx, anchor, tower, prep, want_logits, want_values):
        need = bool(ctx.needs_input_grad[0])   # anchor requires grad <=> grad mode was on at apply() time
        if prep.T > MAX_TILE_SEQ and not tower.training:
            need = False                       # a whole episode in eval mode: forward only, nothing saved (backward() then says so); in train mode run_forward refuses
        logits, values, saved = tower.run_forward(prep, need_grad=need)
        ctx.tower, ctx.prep, ctx.saved = tower, prep, saved
        ctx.want = (want_logits, want_values)
        full = tower._last_full_logits
        ctx.has_full = full is not None
        return logits, values, (full if full is not None else logits.new_zeros(0))

    @staticmethod
    def backward(ctx, dlogits, dvalues, dfull):
        wl, wv = ctx.want
        if ctx.saved is None:
            raise RuntimeError(f"this forward ran without saved activations (T = {ctx.prep.T} > {MAX_TILE_SEQ} steps in eval mode is forward only): no backward")
        ctx.tower.run_backward(ctx.prep, ctx.saved, dlogits.contiguous() if wl else None, dvalues.contiguous() if wv else None,
                               dfull.contiguous() if (wv and ctx.has_full) else None)
        ctx.saved = None
        return None, None, None, None, None


class SafeDinoLLAMATxNavActorCriticSeparate(Tower):
    """Actor tower (= self) + ``critic_tsfm`` + ``c_critic_tsfm`` (separate_actor_critic.py:8-37)."""

    def __init__(self, device="cuda", tokenizer: Optional[GoalTokenizer] = None, max_steps: int = 500,
                 goal_sensor_uuid="natural_language_spec", rgb_dino_preprocessor_uuid="rgb_dinov2",
                 manipulation_rgb_dino_preprocessor_uuid="manipulation_rgb_dinov2", an_object_is_in_hand_uuid="an_object_is_in_hand",
                 time_step_uuid="time_step", traj_idx_uuid="traj_index", critic_type: str = "linear", precision: str = "bf16", full_sensor: bool = True, **unused):
        """``manipulation_rgb_dino_preprocessor_uuid=None`` / ``an_object_is_in_hand_uuid=None``: towers without the manipulation camera / the in-hand sensor, as the
        reference's constructor takes them (allenact_dino_transformer.py:67-68); ``full_sensor=False`` sets both to None, the navigation-only configuration of
        ``DinoV2ViTSTSFMBaseParams.full_sensor`` (dinov2_vits_tsfm_base.py:86,227-232).  The RL towers always embed the previous action (``add_prev_actions=True``)."""
        if not full_sensor:
            manipulation_rgb_dino_preprocessor_uuid = an_object_is_in_hand_uuid = None
        if not torch.cuda.is_available():
            raise RuntimeError("safevla_amd needs an MI355X: there is no CPU or eager fallback for the policy kernels")
        ops.lib()  # fail loudly if the HIP extension is missing
        arena = _Arena()
        device = torch.device(device)
        arena.begin_tower()
        kw = dict(max_steps=max_steps, critic_type=critic_type, precision=precision, in_hand=an_object_is_in_hand_uuid is not None,      # every tower is built from the same kwargs
                  cameras=CAMERAS[:1] if manipulation_rgb_dino_preprocessor_uuid is None else CAMERAS)
        super().__init__(arena, device, **kw)
        arena.begin_tower()
        self.critic_tsfm = Tower(arena, device, **kw)
        arena.begin_tower()
        self.c_critic_tsfm = Tower(arena, device, **kw)
        arena.build(device)
        self.towers = [self, self.critic_tsfm, self.c_critic_tsfm]
        for t in self.towers:
            t.bind()
        self.tokenizer = tokenizer or GoalTokenizer()
        self.uuids = dict(goal=goal_sensor_uuid, nav=rgb_dino_preprocessor_uuid, manip=manipulation_rgb_dino_preprocessor_uuid,
                          hand=an_object_is_in_hand_uuid, time=time_step_uuid, traj=traj_idx_uuid)
        self._anchor = torch.zeros(1, device=device, requires_grad=True)
        # small shapes (acting steps, small-batch updates): towers on concurrent streams; SVLA_SERIAL_TOWERS=1 turns it off
        self.concurrent_towers = os.environ.get("SVLA_SERIAL_TOWERS", "0") != "1"
        self.concurrent_tower_tokens = 1 << 17          # rows x fusion tokens up to which the towers run concurrently
        # Train-mode dropout inside the frozen T5 encoder: by default one realisation per UNIQUE goal per forward (the encoder runs once per
        # unique goal); the reference draws one per (t, b) row (it encodes every row).  True = the reference's statistics, at the price of
        # encoding R rows instead of U unique goals (+13 % FLOPs at L = 12).  Token-id goals only; eval mode is unaffected.
        self._t5_dropout_per_row = False
        # recorded acting steps replay the three towers as grouped launches (ops.GroupedPlans); SVLA_GROUPED_TOWERS=0: the three-stream replay (A/B, tests)
        self.grouped_towers = os.environ.get("SVLA_GROUPED_TOWERS", "1") != "0"
        self._acting_graphs, self._acting_backend = None, "plan"
        self._tower_streams = None                      # one HIP stream per tower (run_towers_concurrently)
        self._invalidate_hooks = []                     # called by invalidate_recorded (the engine's recorded env-chunks)
        if self.concurrent_towers and precision == "bf16" and os.environ.get("SVLA_NO_ACTING_PLANS", "0") != "1":
            self.enable_acting_plans(True)              # recorded single-step launches are the default acting path
        self._goal_cache: Dict[int, List[int]] = {}
        self.sync_weights()

    @property
    def full_sensor(self) -> bool:
        return self.ncam == 2 and self.has_hand

    def mask_non_nav_actions(self):
        """Navigation-only policy: the actor tower's bias of every action outside the reference's navigation set becomes -999999 (dinov2_vits_tsfm_base.py:287-289,
        after the IL checkpoint is loaded), so those actions have probability exactly 0 -- exp(-1e6 - max) underflows to 0 in fp32 -- and are never sampled."""
        from .agent import ALL_STRETCH_ACTIONS, NAV_ACTIONS
        idx = [i for i, a in enumerate(ALL_STRETCH_ACTIONS) if a not in NAV_ACTIONS]
        with torch.no_grad():
            self.actor.linear.bias[torch.as_tensor(idx, device=self.device_)] = -999999.0
        self.sync_weights(frozen=False)
        return idx

    # ---- AllenAct ActorCriticModel API bits -------------------------------------------------------------------
    @property
    def t5_dropout_per_row(self) -> bool:
        """one T5 dropout realisation per (t, b) row and tower, as the reference draws it (default: one per unique goal and pass).  Setting it also pins the frozen
        encoder's RMSNorm form: per-row update passes are too large for the norm-fused small-M GEMM, so the acting steps take the two-launch form too -- rollout
        log-probs and the update's recomputed log-probs then come from the same arithmetic."""
        return self._t5_dropout_per_row

    @t5_dropout_per_row.setter
    def t5_dropout_per_row(self, on: bool) -> None:
        on = bool(on)
        if on != self._t5_dropout_per_row:
            self._t5_dropout_per_row = on
            for t in self.towers:
                t.t5_fused = False if on else None
            self.invalidate_recorded()

    @property
    def recurrent_memory_specification(self):
        return None

    def sampler_select(self, keep: list):
        """AllenAct hook: keep only the listed samplers' KV-cache rows (allenact_dino_transformer.py:197-199)."""
        for t in self.towers:
            t.cache_select(keep)

    def trainable_parameters(self):
        return [p for p in self.parameters() if p.requires_grad]

    # ---- weights ----------------------------------------------------------------------------------------------
    def sync_weights(self, frozen: bool = True):
        """Refresh bf16 mirrors / transposed copies after the fp32 masters changed (load_state_dict, optimiser step)."""
        ar = self.arena
        ops.cast_bf16(ar.flat_p, ar.flat_bf16)
        for t in self.towers:
            t.refresh_transposes()
            if frozen:
                t.visual_encoder.text_encoder.sync(t.adt)
                t._t5_cache = (None, None)
        if frozen:
            # T5Frozen.sync() REPLACES the encoder's runtime tensors: recorded acting steps (and the engine's recorded env-chunks, through
            # the hook below) hold the old ones alive and would keep acting on the previous encoder while updates use the new one
            self.invalidate_recorded()

    def set_fp8_attention(self, on: bool) -> None:
        """BASELINE config 5: run the full-sequence fusion-encoder attention of all three towers (acting and update passes) on the
        e4m3 / e5m2 kernels.  Recorded acting steps are dropped: they hold the other kernels' launches."""
        for t in self.towers:
            t.fp8_attention = bool(on)
        self.invalidate_recorded()

    def invalidate_recorded(self):
        """Drop every recorded launch sequence / captured graph that may reference replaced tensors."""
        if self._acting_graphs is not None:
            self._acting_graphs.clear()
        for hook in self._invalidate_hooks:
            hook()

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        r = super().load_state_dict(state_dict, strict=strict, **kw)
        self.sync_weights()
        return r

    def zero_grad(self, set_to_none: bool = False):
        self.arena.flat_g.zero_()

    # ---- observation preprocessing shared by the towers --------------------------------------------------------
    @torch.no_grad()
    def prepare(self, observations: Dict[str, torch.Tensor], prev_actions: torch.Tensor, masks: torch.Tensor) -> Prep:
        u = self.uuids
        T, B = prev_actions.shape[:2]
        R = T * B
        dev = self.device_
        p = Prep()
        p.T, p.B, p.R = T, B, R
        if "dino_tokens" in observations:       # storage-native layout [T,B,ncam,84,384] bf16
            p.tokens = observations["dino_tokens"].reshape(R, self.ncam, NPATCH, self.dino_dim).to(self.adt).contiguous()
        else:
            p.tokens = torch.empty(R, self.ncam, NPATCH, self.dino_dim, device=dev, dtype=self.adt)
            for cam, key in enumerate((u["nav"], u["manip"])[:self.ncam]):
                ops.feat_to_tokens(observations[key].reshape(R, self.dino_dim, NPATCH).contiguous(), p.tokens, cam, ncam=self.ncam)
        p.prev_actions = prev_actions.reshape(R).contiguous()
        p.masks = masks.reshape(R).to(F32).contiguous()
        p.hand = observations[u["hand"]].reshape(R).contiguous() if self.has_hand else None
        p.time_step = observations[u["time"]].reshape(R).contiguous()
        p.traj_bt = observations[u["traj"]].reshape(T, B).t().contiguous().to(torch.int32)
        # goals: content-hash rows on the GPU, tokenise each unique string once on the host
        per_row = self.t5_dropout_per_row and self.training and "goal_token_ids" in observations
        if "goal_token_ids" in observations and (T == 1 or per_row):
            # single-step (acting) batches: every env is its own goal row -- no de-duplication, hence no host sync (torch.unique), so the
            # host can run ahead of the GPU while it issues the recorded step.  ``t5_dropout_per_row``: the reference's exact train-mode
            # statistics -- it re-encodes the goal of every (t, b) row, so every row sees its own dropout realisation of the frozen T5
            p.ids = observations["goal_token_ids"].reshape(R, -1).contiguous()
            p.attn_mask = (p.ids != 0).to(torch.int64)
            p.attn_mask[:, 0] = 1
            inv = torch.arange(R, device=dev)
        elif "goal_token_ids" in observations:
            ids_rows = observations["goal_token_ids"].reshape(R, -1).contiguous()
            hashes = ops.row_hash(ids_rows.view(torch.uint8).view(R, -1))
            uniq, inv = torch.unique(hashes, return_inverse=True)
            first = torch.full((uniq.numel(),), R, device=dev, dtype=torch.int64).scatter_reduce_(0, inv, torch.arange(R, device=dev), "amin")
            p.ids = ids_rows[first]
            p.attn_mask = (p.ids != 0).to(torch.int64)
            p.attn_mask[:, 0] = 1
        else:
            goal = observations[u["goal"]].reshape(R, -1).contiguous()
            if goal.dtype != torch.uint8:
                goal = goal.to(torch.uint8)
            hashes = ops.row_hash(goal)
            uniq, inv = torch.unique(hashes, return_inverse=True)
            first = torch.full((uniq.numel(),), R, device=dev, dtype=torch.int64).scatter_reduce_(0, inv, torch.arange(R, device=dev), "amin")
            rows = goal[first].cpu().numpy()          # U x 1000 bytes: the only device->host copy of the forward
            keys = uniq.cpu().tolist()
            enc = []
            for k, row in zip(keys, rows):
                if k not in self._goal_cache:
                    self._goal_cache[k] = self.tokenizer.encode(bytes_to_str(row))
                enc.append(self._goal_cache[k])
            L = max(len(e) for e in enc)              # pad to the batch max (reference: padding=True, no fusion mask)
            ids = torch.zeros(len(enc), L, dtype=torch.int64)
            am = torch.zeros(len(enc), L, dtype=torch.int64)
            for i, e in enumerate(enc):
                ids[i, :len(e)] = torch.tensor(e)
                am[i, :len(e)] = 1
            p.ids, p.attn_mask = ids.to(dev), am.to(dev)
            p.ids_key = (tuple(tuple(e) for e in enc), L)      # host-side identity of the goal batch (eval-mode T5 cache)
        p.gid = inv.to(torch.int32).contiguous()
        p.attn_mask_u8 = p.attn_mask.to(torch.uint8).contiguous()      # T5 key-padding mask in the kernels' format (once, not per tower)
        p.U, p.L = p.ids.shape
        p.S = self.text_off + p.L
        return p

    # ---- small shapes: the three (independent) towers on three HIP streams ------------------------------------------------------
    def run_towers_concurrently(self, fn):
        """``[fn(k, tower) for k, tower in enumerate(towers)]`` with tower k issued on its own HIP stream.

        Measured (tools/replay_probe.py): a single-step acting forward is 313 kernels in 4.3 ms whether it is issued eagerly from Python or
        replayed from a pre-bound call list -- it is bound by the GPU-side dispatch of ~100 tiny DEPENDENT kernels per tower (~14 us each),
        not by host issue.  The towers share no intermediate, so running them on three streams overlaps three dependency chains; at
        update-sized shapes (every kernel fills the chip, activations of one tower are tens of GB) the towers stay sequential.
        Inputs were produced on the current stream (side streams wait for it), outputs are handed back to it (it waits for the side
        streams; returned tensors are ``record_stream``-ed so the caching allocator does not recycle them early)."""
        main = torch.cuda.current_stream()
        if self._tower_streams is None:
            self._tower_streams = [torch.cuda.Stream(device=self.device_) for _ in self.towers]
        outs = []
        for k, (t, s) in enumerate(zip(self.towers, self._tower_streams)):
            s.wait_stream(main)
            with torch.cuda.stream(s):
                outs.append(fn(k, t))
        for s in self._tower_streams:
            main.wait_stream(s)

        def _rec(o):
            if isinstance(o, torch.Tensor):
                o.record_stream(main)
            elif isinstance(o, (tuple, list)):
                for x in o:
                    _rec(x)
        _rec(outs)
        return outs

    # ---- captured acting step -------------------------------------------------------------------------------------------
    def enable_acting_graphs(self, on: bool = True, backend: str = "hipgraph"):
        """Single-step (acting) forwards are ~100 small dependent kernels per tower.  With this switch the three-tower step is made
        step-independent -- step counter, KV-cache write slot and dropout seeds in device memory, observations copied into static buffers,
        attention over the whole cache window behind the mask (same kernels, same arithmetic) -- and then either
          backend="plan"     recorded once per (envs, goal length) as three ``ops.LaunchPlan``s (one per tower, each on its own HIP stream)
                             and re-issued from a tight loop: the DEFAULT acting path (``enable_acting_plans``), or
          backend="hipgraph" captured as a HIP graph and replayed: measured slower than eager issue on this ROCm stack, kept opt-in."""
        assert backend in ("plan", "hipgraph")
        self._acting_graphs = {} if on else None
        self._acting_backend = backend

    def enable_acting_plans(self, on: bool = True):
        self.enable_acting_graphs(on, backend="plan")

    def _acting_step_graph(self, prep: Prep):
        B, L = prep.B, prep.L
        plan_mode = self._acting_backend == "plan"
        for t in self.towers:
            t._ensure_caches(B)
        key = (B, L, self.training, self._acting_backend, tuple(t._kv_version for t in self.towers))
        st = self._acting_graphs.get(key)
        dev = self.device_
        if st is None:
            st = _ActingState()
            st.T, st.B, st.R, st.U, st.L, st.S = 1, B, B, B, L, self.text_off + L
            z = lambda *shape, dtype=torch.int64: torch.zeros(*shape, device=dev, dtype=dtype)
            st.tokens, st.prev_actions, st.masks, st.time_step = z(B, self.ncam, NPATCH, self.dino_dim, dtype=self.adt), z(B), z(B, dtype=F32), z(B)
            st.hand = z(B) if self.has_hand else None
            st.traj_bt, st.ids, st.attn_mask = z(B, 1, dtype=torch.int32), z(B, L), torch.ones(B, L, device=dev, dtype=torch.int64)
            st.gid, st.t_dev, st.attn_mask_u8 = torch.arange(B, device=dev, dtype=torch.int32), z(()), torch.ones(B, L, device=dev, dtype=torch.uint8)
            st.kvalid_static = z(B, self.max_steps, dtype=torch.uint8) if plan_mode else None
            st.ar_steps = torch.arange(self.max_steps, device=dev)
            for t in self.towers:
                t._ar_steps = torch.arange(t.max_steps, device=dev)
            for k_old in [k_ for k_ in self._acting_graphs if k_[4] != key[4]]:      # plans of replaced KV caches keep B x max_steps x 1024 x layers x 3 alive
                del self._acting_graphs[k_old]
            self._acting_graphs[key] = st
        for t in self.towers:
            t.refresh_folded()          # (recorded / captured steps do not run the Python that would notice an optimiser step: refresh the gamma-folded weights here, in place)
        # per-step inputs -> static buffers
        st.tokens.copy_(prep.tokens); st.prev_actions.copy_(prep.prev_actions); st.masks.copy_(prep.masks)
        if self.has_hand:
            st.hand.copy_(prep.hand)
        st.time_step.copy_(prep.time_step)
        st.ids.copy_(prep.ids[prep.gid.long()]); st.attn_mask.copy_(prep.attn_mask[prep.gid.long()])
        st.attn_mask_u8.copy_(st.attn_mask)
        st.t_dev.fill_(self.time_step_counter)
        if plan_mode:
            # recorded step: every tower attends to cache slots [max(t - time_step_b, 0), t] (allenact_dino_transformer.py:388-397), computed once
            tc, ar = self.time_step_counter, st.ar_steps
            st.kvalid_static.copy_((ar[None, :] <= tc) & (ar[None, :] >= torch.clamp(tc - st.time_step, min=0)[:, None]))
            for t in self.towers:
                t.advance_device_seed()                  # fresh dropout noise per step: recorded, grouped or three-stream
            if st.plans is None:
                versions = tuple(t._kv_version for t in self.towers)

                def rec(k, t):
                    with ops.LaunchPlan() as plan:
                        return (plan,) + t.static_step(st)
                res = self.run_towers_concurrently(rec)          # the recording pass is a real step
                assert versions == tuple(t._kv_version for t in self.towers)
                st.plans, st.outs = [r[0] for r in res], [(r[1], r[2]) for r in res]
                st.grouped_ok = ops.GroupedPlans.compatible(st.plans)
            elif self.grouped_towers and st.grouped_ok:
                # tower-grouped replay (round 6): call i of the three recorded sequences is issued as ONE grid whose blockIdx.z picks the tower's
                # arguments (csrc/launch.h) -- one dependency chain on the current stream instead of three chains on three streams, three times
                # the workgroups per dispatch.  Same kernels, same arithmetic: bit-identical to the three-stream replay (tests/test_grouped_gpu.py)
                self._grouped_replay(st)
            else:
                # one foreign call per tower (svla_replay_calls), each list on the stream it was recorded on.  Host issue 2.0 -> 1.0 ms per step; the step itself is
                # bound by the GPU side (~310 small dependent kernels on three streams: 3.0 ms), so issuing the three sequences from three host threads -- tried,
                # ctypes drops the GIL during the call -- changes nothing (21.4 k env-steps/s either way)
                self.run_towers_concurrently(lambda k, t: st.plans[k].replay())
            for t in self.towers:
                t.time_step_counter += 1
            return st.outs[0][0].clone(), st.outs[1][1].clone(), st.outs[2][1].clone()

        def body():
            outs = []
            for t in self.towers:
                t.advance_device_seed()                  # fresh dropout noise per replay
                outs.append(t.static_step(st))
            return outs

        if st.graph is None:
            s_ = torch.cuda.Stream()
            s_.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s_):                  # warm-up outside capture (lazy initialisations, allocator)
                body()
            torch.cuda.current_stream().wait_stream(s_)
            st.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(st.graph):
                st.outs = body()
        st.graph.replay()
        for t in self.towers:
            t.time_step_counter += 1
        return st.outs[0][0].clone(), st.outs[1][1].clone(), st.outs[2][1].clone()

    def _grouped_replay(self, st):
        """the recorded step of the three towers as grouped launches on the current stream.  (Issuing the text path -- frozen T5 + text adapter, ~40 small launches that
        leave most CUs idle -- on a side stream next to the visual compressor's GEMMs was measured: 2.324 vs 2.321 ms per step, not kept.)"""
        main = torch.cuda.current_stream()
        gp = st.gplans.get(main.cuda_stream)
        if gp is None:
            gp = st.gplans[main.cuda_stream] = ops.GroupedPlans(st.plans, main.cuda_stream)
        gp.replay()

    def _acting_fast(self, observations, prev_actions, masks):
        """A recorded, tower-grouped step issued straight from the observation dict: ONE staging launch (svla_acting_stage: inputs -> static buffers, T5 padding masks,
        KV-window mask, step counter, seed bumps) + the grouped replay -- no ``prepare``, none of the ~30 framework copies / compares the general path spends on a
        step.  Returns None whenever anything is not exactly as the recorded step expects (first step of a shape, other dtypes / layouts, string goals, a cache
        window about to wrap): the general path then handles -- and, if needed, records -- the step."""
        if self._acting_graphs is None or self._acting_backend != "plan" or not self.grouped_towers or torch.is_grad_enabled():
            return None
        tk, ids = observations.get("dino_tokens"), observations.get("goal_token_ids")
        if tk is None or ids is None or prev_actions.dim() != 2 or prev_actions.shape[0] != 1:
            return None
        B, L, tc = prev_actions.shape[1], ids.shape[-1], self.time_step_counter
        if not (tc < self.max_steps - 1 and all(t.time_step_counter == tc and t._kv is not None and t._kv[0].shape[0] >= B for t in self.towers)):
            return None
        st = self._acting_graphs.get((B, L, self.training, self._acting_backend, tuple(t._kv_version for t in self.towers)))
        if st is None or st.plans is None or not st.grouped_ok:
            return None
        u = self.uuids
        hand, ts = (observations.get(u["hand"]) if self.has_hand else None), observations.get(u["time"])      # no in-hand sensor: nothing is read, the stage gets a NULL pair
        i64 = torch.int64
        if (self.has_hand and hand is None) or ts is None or not (tk.dtype == self.adt and tk.is_contiguous() and tk.numel() == st.tokens.numel() and prev_actions.dtype == i64 and prev_actions.is_contiguous()
                                              and masks.dtype == F32 and masks.is_contiguous() and masks.numel() == B and (hand is None or (hand.dtype == i64 and hand.is_contiguous() and hand.numel() == B))
                                              and ts.dtype == i64 and ts.is_contiguous() and ts.numel() == B and ids.dtype == i64 and ids.is_contiguous() and ids.numel() == B * L):
            return None
        for t in self.towers:
            t.refresh_folded()
        ops.acting_stage(tk, st.tokens, prev_actions, st.prev_actions, masks, st.masks, hand, st.hand, ts, st.time_step, ids, st.ids, st.attn_mask, st.attn_mask_u8,
                         st.kvalid_static, st.t_dev, B, L, self.max_steps, tc, [t._seed_dev_buf for t in self.towers], SEED_STEP)
        self._grouped_replay(st)
        for t in self.towers:
            t.time_step_counter += 1
        return SafeActorCriticOutput(distributions=CategoricalDistr(st.outs[0][0].clone()), values=st.outs[1][1].clone(), c_values=st.outs[2][1].clone(), extras={})

    # ---- reference forward API -------------------------------------------------------------------------------------
    def forward(self, observations, memory, prev_actions, masks):
        fast = self._acting_fast(observations, prev_actions, masks)
        if fast is not None:
            return fast, memory
        for t in self.towers:      # sequences above MAX_TILE_SEQ steps: forward only, refused before the first launch where they cannot run
            t._check_seq_len(int(prev_actions.shape[0]), torch.is_grad_enabled() and self.training)
        prep = self.prepare(observations, prev_actions, masks)
        if (prep.T == 1 and self._acting_graphs is not None and not torch.is_grad_enabled()
                and self.time_step_counter < self.max_steps - 1 and all(t.time_step_counter == self.time_step_counter for t in self.towers)):
            logits, values, c_values = self._acting_step_graph(prep)
            return SafeActorCriticOutput(distributions=CategoricalDistr(logits), values=values, c_values=c_values, extras={}), memory
        if prep.T == 1 and torch.is_grad_enabled():
            raise RuntimeError("single-step (acting) forwards run under torch.no_grad(), as in the reference's rollout collection")
        if not torch.is_grad_enabled() and self.concurrent_towers and prep.R * prep.S <= self.concurrent_tower_tokens:
            (logits, _), (_, values), (_, c_values) = self.run_towers_concurrently(lambda k, t: t.run_forward(prep, need_grad=False)[:2])
            c_full = self.c_critic_tsfm._last_full_logits
        else:
            logits, _, _ = _TowerFn.apply(self._anchor, self, prep, True, False)
            _, values, _ = _TowerFn.apply(self._anchor, self.critic_tsfm, prep, False, True)
            _, c_values, c_full = _TowerFn.apply(self._anchor, self.c_critic_tsfm, prep, False, True)
        # the diagnostics in ``extras`` are consumed by the losses only (update batches); single-step acting forwards skip them
        extras = self._extras(c_values, c_full) if prep.T > 1 else {}
        return SafeActorCriticOutput(distributions=CategoricalDistr(logits), values=values, c_values=c_values, extras=extras), memory

    def _extras(self, c_values, c_full=None):
        """``extras`` of the COST-critic tower, which is what the 3-tower wrapper hands on (separate_actor_critic.py:31-36); keys per
        allenact_dino_transformer.py:425-463: total_norm (the tower's gradient norm as left by the previous backward), stop_grad_values
        (or stop_grad_logits / full_logits / loss_func for the discrete critic), weight_norm / bias_norm / weight_grad_norm of the last
        critic layer.  Device tensors (the reference builds host tensors with one sync each)."""
        tw = self.c_critic_tsfm
        with torch.no_grad():
            fc = tw.critic.fc if tw.critic_type == "linear" else tw.critic.fc[-1]
            a, b = self.arena.tower_ranges[2]
            sq = torch.zeros(1, device=self.device_, dtype=torch.float64)
            ops.sumsq(self.arena.flat_g[a:b], sq)
            extras = {"total_norm": sq.sqrt().float(), "weight_norm": fc.weight.norm(2).reshape(1), "bias_norm": fc.bias.norm(2).reshape(1),
                      "weight_grad_norm": tw.g(fc.weight).norm(2).reshape(1)}
        if tw.critic_type == "discrete" and c_full is not None and c_full.numel():
            extras.update(full_logits=c_full, stop_grad_logits=c_full.detach(), loss_func=tw.critic.loss_fn)
        else:
            extras["stop_grad_values"] = c_values.detach()
        return extras
