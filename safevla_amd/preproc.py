"""Frozen-ViT sensor preprocessors (rollout time), mirroring the reference's preprocessor contract
``process(obs: Dict[str, Tensor]) -> Tensor`` with attributes ``input_uuids`` / ``uuid``:

  * ``DataAugmentationPreprocessor``  /root/reference/architecture/allenact_preprocessors/dino_preprocessors.py:166-239
    (u8 HWC -> /255, -mean, /std; with use_augmentation the sampled v2 transform of utils/transformation_util.py runs first, as u8 kernels)
  * ``DinoViTPreprocessor`` / ``DinoViTEmbedder``  dino_preprocessors.py:20-125: crop W 384 -> 378, DINOv2 ViT-S/14
    ``forward_features(...)["x_norm_patchtokens"]`` -> (B,384,16,27) -> AdaptiveAvgPool2d((7,12)).

The DINOv2 network itself is third-party (``torch.hub facebookresearch/dinov2``, not in the reference tree, no network
here): its published ViT-S/14 forward is restated (pre-LN blocks with qkv/proj biases, LayerScale, GELU MLP, final LayerNorm,
bicubic position-embedding interpolation) with the hub model's ``state_dict`` names, random-init geometry. PARITY UNPINNED
against DINOv2 proper; pinned against the fp32 oracle restatement (oracle/ref_vit.py).

Geometry-generic: DINOv2 ViT-S/B/L-14 (widths 384 / 768 / 1024, 433 tokens) and the SigLIP ViT-B/L-16 trunk
(256 tokens, no class token) run on the same kernels -- ``SigLIPPreprocessor`` mirrors siglip_preprocessors.py:18-104.

The CLIP RN50 conv trunk of ``clip_resnet_50_3`` (``ClipResNet`` / ``ClipResNetPreprocessor`` below; image_encoders.py:11-48) is the one convolutional encoder:
stem + 16 bottlenecks on the implicit-GEMM convolution of csrc/conv.hip, eval-mode BatchNorm folded into the weights at sync time.

MI355X path: normalise + crop + im2col fused in one kernel, patch embedding and all block linears on the bf16 MFMA GEMM
(LayerScale folded into the frozen weights at sync time), fused attention at S = 433, output written directly in the rollout
storage's bf16 token layout [B, ncam, 84, 384] (and/or the reference's fp32 (B,384,7,12)).
"""
import functools
import math
import random
from typing import Dict, NamedTuple, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .api import Box
from .model import _NS

DINO_RGB_MEANS = (0.48145466, 0.4578275, 0.40821073)
DINO_RGB_STDS = (0.26862954, 0.26130258, 0.27577711)
BF16 = torch.bfloat16


# ---- sampled frame augmentation: host side (no device needed) -------------------------------------------------------------------
# The reference samples ONE concrete transform from the v2 list (utils/transformation_util.py:12-28) with Python's ``random`` (sample_a_specific_transform,
# :54-119), keeps it for num_steps_to_change calls of DataAugmentationPreprocessor.process (dino_preprocessors.py:224-231) and applies it to the whole batch.
# What torchvision still draws per call with fixed factors -- the order of the four ColorJitter operations and the crop box -- is drawn here per call on a
# torch generator.  The kernels (csrc/augment.hip) take everything as arguments.
AUG_BRIGHTNESS, AUG_CONTRAST, AUG_SATURATION, AUG_HUE = ops.AUG_BRIGHTNESS, ops.AUG_CONTRAST, ops.AUG_SATURATION, ops.AUG_HUE
AUG_STAGES = ("jitter0", "jitter1", "jitter2", "jitter3", "blur", "crop_resize", "posterize", "sharpness")


class AugmentParams(NamedTuple):
    brightness: float
    saturation: float
    hue: float
    contrast: float
    sigma: float
    scale: float
    posterize_draws: Tuple[int, int, int, int]
    sharpness: int

    @property
    def posterize(self) -> bool:
        """every RandomPosterize entry is rebuilt with bits = 7 (transformation_util.py:101-103): clearing the low bit is idempotent, so the four entries
        reduce to: clear it if any of the four draws is 1"""
        return any(self.posterize_draws)

    def factor(self, op: int) -> float:
        return (self.brightness, self.contrast, self.saturation, self.hue)[op]


def sample_augment_params(rng=random) -> AugmentParams:
    """sample_a_specific_transform on the v2 list, in its draw order (ColorJitter: brightness, saturation, hue, contrast; blur sigma; crop scale; four posterize
    draws; one sharpness draw).  ``rng``: the ``random`` module or a ``random.Random``."""
    brightness = rng.uniform(0.6, 1.4)          # ColorJitter(brightness=0.4) -> [1 - 0.4, 1 + 0.4]
    saturation = rng.uniform(0.8, 1.2)
    hue = rng.uniform(-0.05, 0.05)
    contrast = rng.uniform(0.6, 1.4)
    sigma = rng.uniform(0.1, 2)
    scale = rng.uniform(0.9, 1)
    post = tuple(int(rng.random() < 0.2) for _ in range(4))
    sharp = int(rng.random() < 0.5)
    return AugmentParams(brightness, saturation, hue, contrast, sigma, scale, post, sharp)


CROP_RATIO = (3.0 / 4.0, 4.0 / 3.0)


def crop_attempts_can_succeed(H: int, W: int, scale: float, ratio=CROP_RATIO) -> bool:
    """False only when no aspect ratio in ``ratio`` gives a box of area scale * H * W inside H x W (then every attempt of the search fails and the box is the
    centre-crop fallback: at 224 x 384 the crop height is at least round(sqrt(0.9 * 86016 * 3/4)) = 241 > 224)."""
    area = H * W * scale
    r_lo = max(ratio[0], area / (H + 0.5) ** 2)      # h = round(sqrt(area / r)) <= H needs r >= area / (H + 0.5)^2
    r_hi = min(ratio[1], (W + 0.5) ** 2 / area)      # w = round(sqrt(area * r)) <= W needs r <= (W + 0.5)^2 / area
    return r_lo <= r_hi * (1 + 1e-6)


def crop_box(H: int, W: int, scale: float, generator: Optional[torch.Generator] = None, ratio=CROP_RATIO) -> Tuple[int, int, int, int]:
    """RandomResizedCrop's parameter search with the scale range collapsed to the sampled value: ten attempts with a log-uniform aspect ratio, then the
    centre-crop fallback.  Returns (top, left, height, width)."""
    area = H * W
    if crop_attempts_can_succeed(H, W, scale, ratio):
        lo, hi = math.log(ratio[0]), math.log(ratio[1])
        for _ in range(10):
            target = area * scale
            ar = math.exp(torch.empty(1).uniform_(lo, hi, generator=generator).item())
            w, h = int(round(math.sqrt(target * ar))), int(round(math.sqrt(target / ar)))
            if 0 < w <= W and 0 < h <= H:
                top = int(torch.randint(0, H - h + 1, (1,), generator=generator).item())
                left = int(torch.randint(0, W - w + 1, (1,), generator=generator).item())
                return top, left, h, w
    return crop_fallback_box(H, W, ratio)


def crop_fallback_box(H: int, W: int, ratio=CROP_RATIO) -> Tuple[int, int, int, int]:
    """RandomResizedCrop's centre crop when no attempt of the search fits: the whole frame clipped to the nearer end of ``ratio``"""
    in_ratio = float(W) / float(H)
    if in_ratio < min(ratio):
        w = W
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = H
        w = int(round(h * max(ratio)))
    else:
        w, h = W, H
    h, w = min(h, H), min(w, W)
    return (H - h) // 2, (W - w) // 2, h, w


@functools.lru_cache(maxsize=64)
def gaussian_weights(ksize: int, sigma: float) -> Tuple[float, ...]:
    """normalised 1-D weights exp(-0.5 (x / sigma)^2) on the integer offsets of a ``ksize``-tap kernel, computed in fp32"""
    half = (ksize - 1) * 0.5
    x = torch.linspace(-half, half, ksize, dtype=torch.float32)
    pdf = torch.exp(-0.5 * (x / torch.tensor(sigma, dtype=torch.float32)).pow(2))
    return tuple((pdf / pdf.sum()).tolist())


class AugmentCall(NamedTuple):
    """everything one call applies: the sampled transform, this call's ColorJitter order and crop box"""
    params: AugmentParams
    order: Tuple[int, int, int, int]
    box: Tuple[int, int, int, int]


def apply_augment_u8(x: torch.Tensor, call: AugmentCall, debug: bool = False, out: Optional[torch.Tensor] = None):
    """u8 [B,H,W,3] -> u8 [B,H,W,3]: ColorJitter in the call's order, blur, crop + resize, posterize, sharpness.
    Product form: three launches (gray partial sums of the image entering contrast; jitter + blur; resize + posterize + sharpness).
    ``debug``: every stage in a launch of its own; returns [(stage name, u8 image)] for the eight stages of AUG_STAGES (a stage that was not sampled
    returns its input)."""
    p, order = call.params, list(call.order)
    factors = [p.factor(o) for o in order]
    wx, wy = gaussian_weights(5, p.sigma), gaussian_weights(9, p.sigma)
    if not debug:
        k = order.index(AUG_CONTRAST)
        part = ops.aug_gray_partials(x, order[:k], factors[:k])
        y = ops.aug_jitter_blur(x, order, factors, part, wx, wy)
        return ops.aug_resize_post_sharp(y, call.box, p.posterize, bool(p.sharpness), out=out)
    stages = []
    for i, (o, f) in enumerate(zip(order, factors)):
        part = ops.aug_gray_partials(x) if o == AUG_CONTRAST else None
        x = ops.aug_jitter_blur(x, [o], [f], part)
        stages.append((AUG_STAGES[i], x))
    x = ops.aug_jitter_blur(x, wx=wx, wy=wy)
    stages.append(("blur", x))
    x = ops.aug_resize_post_sharp(x, call.box)
    stages.append(("crop_resize", x))
    if p.posterize:
        x = ops.aug_resize_post_sharp(x, posterize=True)
    stages.append(("posterize", x))
    if p.sharpness:
        x = ops.aug_resize_post_sharp(x, sharpen=True)
    stages.append(("sharpness", x))
    return stages


# ---- the full random v2 list, per trajectory (imitation-learning training from raw frames) ----------------------------------------------------
# The IL Preprocessor (architecture/models/transformer_models/preprocessors.py:86-118) builds tensor_image_preprocessor(data_augmentation=True) with specific=False
# (:22-60): the random v2 list of utils/transformation_util.py:12-28 itself, applied once per trajectory and camera to that trajectory's [T, 3, H, W] frames.  Every
# call draws everything anew -- ColorJitter order and factors, blur sigma, a crop box with its own scale, four posterize coins (7, 6, 5, 4 bits), one sharpness coin.
CROP_SCALE = (0.9, 1.0)
POSTERIZE_BITS = (7, 6, 5, 4)


class RandomAugmentCall(NamedTuple):
    """one call of the random v2 list: what it drew, in the form the grouped kernels take"""
    order: Tuple[int, int, int, int]
    brightness: float
    contrast: float
    saturation: float
    hue: float
    sigma: float
    box: Tuple[int, int, int, int]
    post_mask: int
    sharpen: bool

    def factor(self, op: int) -> float:
        return (self.brightness, self.contrast, self.saturation, self.hue)[op]

    def as_augment_call(self) -> AugmentCall:
        """the same transform for the single-transform path (apply_augment_u8), which knows posterize to 7 bits only"""
        assert self.post_mask in (0xFF, 0xFE), f"apply_augment_u8 cannot express post_mask {self.post_mask:#x}"
        p = AugmentParams(self.brightness, self.saturation, self.hue, self.contrast, self.sigma, 1.0, (int(self.post_mask == 0xFE), 0, 0, 0), int(self.sharpen))
        return AugmentCall(p, self.order, self.box)


def posterize_mask(coins) -> int:
    """the chain RandomPosterize(7), (6), (5), (4) with the coins that came up: x & m7 & m6 ... = x & (0xFF << (8 - the fewest bits drawn)); none drawn: 0xFF"""
    bits = [b for b, c in zip(POSTERIZE_BITS, coins) if c]
    return (0xFF << (8 - min(bits))) & 0xFF if bits else 0xFF


def sample_random_augment_call(H: int, W: int, generator: Optional[torch.Generator] = None, ratio=CROP_RATIO) -> RandomAugmentCall:
    """The per-call draws of the random v2 list on a torch generator, in Compose order (torchvision is not installed here: this sequence is the contract, PARITY
    UNPINNED like the sampler above).  ColorJitter: randperm(4), then brightness, contrast, saturation, hue.  GaussianBlur: sigma.  RandomResizedCrop: up to ten
    attempts, each drawing a scale and a log-uniform ratio (both consumed whether or not the attempt can fit), top and left on success, else the centre-crop
    fallback.  RandomPosterize x 4: one coin each for 7, 6, 5, 4 bits.  RandomAdjustSharpness: one coin."""
    g = generator
    u = lambda lo, hi: torch.empty(1).uniform_(lo, hi, generator=g).item()
    order = tuple(int(v) for v in torch.randperm(4, generator=g).tolist())
    brightness, contrast, saturation, hue = u(0.6, 1.4), u(0.6, 1.4), u(0.8, 1.2), u(-0.05, 0.05)
    sigma = u(0.1, 2.0)
    box = None
    lo, hi = math.log(ratio[0]), math.log(ratio[1])
    for _ in range(10):
        target = H * W * u(*CROP_SCALE)
        ar = math.exp(u(lo, hi))
        w, h = int(round(math.sqrt(target * ar))), int(round(math.sqrt(target / ar)))
        if 0 < w <= W and 0 < h <= H:
            top = int(torch.randint(0, H - h + 1, (1,), generator=g).item())
            left = int(torch.randint(0, W - w + 1, (1,), generator=g).item())
            box = (top, left, h, w)
            break
    if box is None:
        box = crop_fallback_box(H, W, ratio)
    coins = [bool(torch.rand(1, generator=g).item() < 0.2) for _ in POSTERIZE_BITS]
    sharpen = bool(torch.rand(1, generator=g).item() < 0.5)
    return RandomAugmentCall(order, brightness, contrast, saturation, hue, sigma, box, posterize_mask(coins), sharpen)


def apply_random_augment_u8(x: torch.Tensor, calls, group_len: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """u8 [N,H,W,3] -> u8 [N,H,W,3]: frame n gets ``calls[n // group_len]`` (RandomAugmentCall) -- ColorJitter in that call's order, its blur, its crop + resize, its
    posterize mask, its sharpness.  Three launches (each uploads the table it validated) whatever len(calls) is; per frame bit for bit what apply_augment_u8 computes with the same
    transform.  A refused table (ops.aug_*_grouped) raises before anything is launched: ``out`` stays untouched."""
    table = ops.AugTable([(c.order, [c.factor(o) for o in c.order], gaussian_weights(5, c.sigma), gaussian_weights(9, c.sigma), c.box, c.post_mask, c.sharpen)
                          for c in calls], x.device)
    part = ops.aug_gray_partials_grouped(x, table, group_len)
    y = ops.aug_jitter_blur_grouped(x, table, group_len, part)
    return ops.aug_resize_post_sharp_grouped(y, table, group_len, out=out)


class RandomDataAugmenter:
    """The IL Preprocessor's frame augmentation (preprocessors.py:101-118) for one camera: ``augment_u8`` draws one random call per trajectory of a
    [B, T, H, W, 3] uint8 batch and applies the B transforms in one grouped application (group = trajectory).  ``size``: the model's input size when it is not the
    camera's (the SigLIP presets' (256, 256)): the antialiased bicubic resize runs first and the list acts at the resized geometry, as the reference builds it
    with ``size``.  ``generator``: torch generator of the draws; None = the CPU default.  ``last_calls``: the calls of the latest batch."""

    def __init__(self, size: Optional[Tuple[int, int]] = None, generator: Optional[torch.Generator] = None):
        self.size = None if size is None else (int(size[0]), int(size[1]))
        self.generator = generator
        self.last_calls = []

    def augment_u8(self, frames_u8: torch.Tensor) -> torch.Tensor:
        assert frames_u8.dtype == torch.uint8 and frames_u8.dim() == 5 and frames_u8.shape[-1] == 3, f"uint8 [B,T,H,W,3] frames; got {tuple(frames_u8.shape)}"
        B, T = frames_u8.shape[:2]
        x = frames_u8.reshape(B * T, *frames_u8.shape[2:]).contiguous()
        if self.size is not None and tuple(x.shape[1:3]) != self.size:
            x = ops.resize_bicubic_aa_u8(x, self.size)
        H, W = x.shape[1:3]
        self.last_calls = [sample_random_augment_call(H, W, self.generator) for _ in range(B)]
        return apply_random_augment_u8(x, self.last_calls, T).view(B, T, H, W, 3)


class DataAugmentationPreprocessor:
    """dino_preprocessors.py:166-239.  ``use_augmentation=True`` (the reference's default, training/online/dinov2_vits_tsfm_base.py:62,124,152): one transform
    sampled on the first call and every ``num_steps_to_change`` calls after it, applied to the whole batch as u8 kernels before the normalisation.  Each
    camera's preprocessor owns its transform.  ``generator``: torch generator of the per-call draws (ColorJitter order, crop box); None = the CPU default."""

    def __init__(self, rgb_input_uuid: str, output_uuid: str, device="cuda", normalize=True, mean=DINO_RGB_MEANS, stdev=DINO_RGB_STDS,
                 height=224, width=384, use_augmentation=False, num_steps_to_change=500, generator: Optional[torch.Generator] = None, **kw):
        self.input_uuids, self.uuid, self.device = [rgb_input_uuid], output_uuid, torch.device(device)
        self.mean, self.stdev, self.normalize = mean, stdev, normalize
        self.observation_space = Box(-float("inf"), float("inf"), (height, width, 3))        # dino_preprocessors.py:205-214
        self.use_augmentation = bool(use_augmentation)
        if self.use_augmentation:
            assert num_steps_to_change >= 1
            self.num_steps_to_change, self.num_steps = int(num_steps_to_change), 0
            self.augmentations: Optional[AugmentParams] = None
            self.generator = generator

    def to(self, device):
        self.device = torch.device(device)
        return self

    def next_call(self, H: int, W: int) -> AugmentCall:
        """advance the schedule by one call (dino_preprocessors.py:226-228) and draw what this call draws.  Host only."""
        assert self.use_augmentation, "constructed with use_augmentation=False"
        if self.num_steps == 0 or self.augmentations is None:
            self.augmentations = sample_augment_params()
        self.num_steps = (self.num_steps + 1) % self.num_steps_to_change
        order = tuple(int(v) for v in torch.randperm(4, generator=self.generator).tolist())
        return AugmentCall(self.augmentations, order, crop_box(H, W, self.augmentations.scale, self.generator))

    def _frames(self, frames_u8):
        x = frames_u8.to(self.device)
        assert x.dtype == torch.uint8 and x.dim() == 4 and x.shape[-1] == 3
        return x.contiguous()

    def augment_u8(self, frames_u8: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """u8 [B,H,W,3] -> augmented u8 [B,H,W,3]; counts as one call of the schedule"""
        x = self._frames(frames_u8)
        return apply_augment_u8(x, self.next_call(x.shape[1], x.shape[2]), out=out)

    def augment_u8_stages(self, frames_u8: torch.Tensor):
        """debug form of augment_u8: (AugmentCall, [(stage name, u8 image after that stage)]), one launch per stage; counts as one call of the schedule"""
        x = self._frames(frames_u8)
        call = self.next_call(x.shape[1], x.shape[2])
        return call, apply_augment_u8(x, call, debug=True)

    def process(self, obs: Dict[str, torch.Tensor], *a, **k) -> torch.Tensor:
        x = obs[self.input_uuids[0]].to(self.device)
        assert x.dtype == torch.uint8 and x.shape[-1] == 3
        x = x.contiguous()
        if self.use_augmentation:
            x = self.augment_u8(x)
        return ops.normalize_u8(x, self.mean if self.normalize else (0, 0, 0), self.stdev if self.normalize else (1, 1, 1))


SIGLIP_RGB_MEANS, SIGLIP_RGB_STDS = (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)


class SigLIPDataAugmentationPreprocessor(DataAugmentationPreprocessor):
    """The camera-frame front of the SigLIP presets: ``tensor_image_preprocessor(size=(256, 256))`` of preprocessors.py:22-60 as the IL ``SigLipPreprocessor``
    (:319-328) and the online ``DataAugmentationPreprocessor`` of siglip_preprocessors.py:144-210 use it.  Frames whose size is not ``size`` go through
    torchvision's ``Resize(size, bicubic, antialias=True)`` first (one launch, ``ops.resize_bicubic_aa_u8``: fp32 interpolation of the uint8 frames, clamp, round,
    uint8); frames that already have it pass through untouched.  With ``use_augmentation`` the sampled v2 transform then runs at the resized geometry -- the
    reference builds the list with ``size=(256, 256)``, so its crop box and blur act on the 256 x 256 image -- and ``/255`` with ``Normalize(mean, stdev)`` follow.

    ``augment_u8`` makes this class an ``augmenter=`` of ``SigLIPPreprocessor``, whose own input stays 256 x 256.

    ``random_per_call=True`` (with ``use_augmentation``) is the reference's online SigLIP class as written: the FULL random v2 list drawn afresh on every call,
    including its four-step posterize chain with bits 7 to 4 -- one ``sample_random_augment_call`` per ``process`` / ``augment_u8``, applied to the whole batch as one
    group (the grouped launches with G = 1).  The default keeps the sampled-specific list (one transform kept for ``num_steps_to_change`` calls, posterize to 7
    bits), as the DINOv2 preprocessor's augmentation does."""

    def __init__(self, rgb_input_uuid: str, output_uuid: str, device="cuda", height=224, width=384, size=(256, 256), mean=SIGLIP_RGB_MEANS, stdev=SIGLIP_RGB_STDS,
                 normalize=True, use_augmentation=False, num_steps_to_change=500, generator: Optional[torch.Generator] = None, random_per_call=False, **kw):
        super().__init__(rgb_input_uuid, output_uuid, device=device, normalize=normalize, mean=mean, stdev=stdev, height=height, width=width,
                         use_augmentation=use_augmentation, num_steps_to_change=num_steps_to_change, generator=generator)
        self.size = (int(size[0]), int(size[1]))
        self.observation_space = Box(-float("inf"), float("inf"), (*self.size, 3))
        self.random_per_call = bool(random_per_call)
        self.last_random_call: Optional[RandomAugmentCall] = None

    def augment_u8(self, frames_u8: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """u8 [B,H,W,3] -> u8 [B,*size,3]: resize when the size differs, then (use_augmentation) the sampled transform, which counts as one call of the schedule"""
        x = self._frames(frames_u8)
        resize = tuple(x.shape[1:3]) != self.size
        if not self.use_augmentation:
            if resize:
                return ops.resize_bicubic_aa_u8(x, self.size, out=out)
            if out is None:
                return x
            out.copy_(x)
            return out
        if resize:
            x = ops.resize_bicubic_aa_u8(x, self.size)
        if self.random_per_call:
            self.last_random_call = sample_random_augment_call(*self.size, self.generator)
            return apply_random_augment_u8(x, [self.last_random_call], x.shape[0], out=out)
        return apply_augment_u8(x, self.next_call(*self.size), out=out)

    def augment_u8_stages(self, frames_u8: torch.Tensor):
        assert not self.random_per_call, "the stage-by-stage debug form exists for the sampled-specific transform only"
        x = self._frames(frames_u8)
        if tuple(x.shape[1:3]) != self.size:
            x = ops.resize_bicubic_aa_u8(x, self.size)
        call = self.next_call(*self.size)
        return call, apply_augment_u8(x, call, debug=True)

    def process(self, obs: Dict[str, torch.Tensor], *a, **k) -> torch.Tensor:
        x = self.augment_u8(obs[self.input_uuids[0]])
        return ops.normalize_u8(x, self.mean if self.normalize else (0, 0, 0), self.stdev if self.normalize else (1, 1, 1))


# geometry presets: (dim, depth, heads, patch, native_grid, class token, LayerScale)
VIT_PRESETS = {
    # DINOv2 (torch.hub facebookresearch/dinov2; dino_preprocessors.py:14-18,54-76): pos_embed is the 37 x 37 grid of 518 / 14
    "dinov2_vits14": dict(dim=384, depth=12, heads=6, patch=14, native_grid=37, cls=True, layerscale=True),
    "dinov2_vitb14": dict(dim=768, depth=12, heads=12, patch=14, native_grid=37, cls=True, layerscale=True),
    "dinov2_vitl14": dict(dim=1024, depth=24, heads=16, patch=14, native_grid=37, cls=True, layerscale=True),
    # timm trunk of hf-hub:timm/ViT-B-16-SigLIP-256 (siglip_preprocessors.py:15,86-88; image_encoders.py:75-112): 256 x 256 input,
    # 16 x 16 patches -> 256 tokens, no class token, no LayerScale, learned [1, 256, 768] position embedding used as is
    "ViT-B-16-SigLIP-256": dict(dim=768, depth=12, heads=12, patch=16, native_grid=16, cls=False, layerscale=False),
    "ViT-L-16-SigLIP-256": dict(dim=1024, depth=24, heads=16, patch=16, native_grid=16, cls=False, layerscale=False),
}


class DinoViT(nn.Module):
    """Frozen ViT trunk with the hub / timm parameter names: DINOv2 ViT-S/B/L-14 and the SigLIP ViT-B/L-16 geometries."""

    def __init__(self, device, dim=384, depth=12, heads=6, patch=14, native_grid=37, cls=True, layerscale=True):
        super().__init__()
        assert dim % 64 == 0 and dim // heads == 64, "attention kernels: head_dim 64"
        self.dim, self.depth, self.heads, self.patch, self.native_grid = dim, depth, heads, patch, native_grid
        self.has_cls, self.has_ls = cls, layerscale
        d = torch.device(device)
        P = lambda *s, sc=0.02: nn.Parameter((torch.randn(*s) * sc).to(d), requires_grad=False)
        if cls:
            self.cls_token = P(1, 1, dim)
            self.mask_token = P(1, dim)
        self.pos_embed = P(1, (1 if cls else 0) + native_grid * native_grid, dim)
        self.patch_embed = _NS(); self.patch_embed.proj = _NS()
        self.patch_embed.proj.weight = P(dim, 3, patch, patch, sc=1.0 / math.sqrt(3 * patch * patch))
        self.patch_embed.proj.bias = P(dim)
        self.blocks = nn.ModuleList()
        for _ in range(depth):
            b = _NS()
            b.norm1 = _NS(); b.norm1.weight = nn.Parameter(torch.ones(dim, device=d), requires_grad=False); b.norm1.bias = P(dim)
            b.attn = _NS(); b.attn.qkv = _NS(); b.attn.proj = _NS()
            b.attn.qkv.weight = P(3 * dim, dim, sc=1.0 / math.sqrt(dim)); b.attn.qkv.bias = P(3 * dim)
            b.attn.proj.weight = P(dim, dim, sc=1.0 / math.sqrt(dim)); b.attn.proj.bias = P(dim)
            if layerscale:
                b.ls1 = _NS(); b.ls1.gamma = nn.Parameter(torch.full((dim,), 1.0, device=d), requires_grad=False)
            b.norm2 = _NS(); b.norm2.weight = nn.Parameter(torch.ones(dim, device=d), requires_grad=False); b.norm2.bias = P(dim)
            b.mlp = _NS(); b.mlp.fc1 = _NS(); b.mlp.fc2 = _NS()
            b.mlp.fc1.weight = P(4 * dim, dim, sc=1.0 / math.sqrt(dim)); b.mlp.fc1.bias = P(4 * dim)
            b.mlp.fc2.weight = P(dim, 4 * dim, sc=1.0 / math.sqrt(4 * dim)); b.mlp.fc2.bias = P(dim)
            if layerscale:
                b.ls2 = _NS(); b.ls2.gamma = nn.Parameter(torch.full((dim,), 1.0, device=d), requires_grad=False)
            self.blocks.append(b)
        self.norm = _NS(); self.norm.weight = nn.Parameter(torch.ones(dim, device=d), requires_grad=False); self.norm.bias = P(dim)
        self._rt = None

    def interpolated_pos(self, gh: int, gw: int) -> torch.Tensor:
        """[(1 +) gh*gw, dim] fp32: class position + bicubic resize of the native_grid^2 patch positions (DINOv2 interpolate_pos_encoding);
        the native grid is used as is (SigLIP at its own 16 x 16)."""
        pe = self.pos_embed[0].float()
        g, nc = self.native_grid, (1 if self.has_cls else 0)
        if (gh, gw) == (g, g):
            return pe.contiguous()
        patch = pe[nc:].reshape(1, g, g, self.dim).permute(0, 3, 1, 2)
        patch = F.interpolate(patch, size=(gh, gw), mode="bicubic", align_corners=False)
        return torch.cat([pe[:nc], patch.permute(0, 2, 3, 1).reshape(gh * gw, self.dim)], 0).contiguous()

    def sync(self, gh=16, gw=27, KP=None):
        K = 3 * self.patch * self.patch
        KP = KP or ((K + 31) // 32) * 32          # im2col rows padded to the GEMM's K granule (588 -> 608; 768 stays)
        rt = dict(gh=gh, gw=gw, KP=KP)
        w = self.patch_embed.proj.weight.reshape(self.dim, -1).float()
        wp = torch.zeros(self.dim, KP, device=w.device)
        wp[:, : w.shape[1]] = w
        rt["pe_w"] = wp.to(BF16).contiguous()
        rt["pe_b"] = self.patch_embed.proj.bias.float().contiguous()
        rt["pos"] = self.interpolated_pos(gh, gw)
        rt["cls"] = self.cls_token.reshape(-1).float().contiguous() if self.has_cls else None
        blocks = []
        one = torch.ones(self.dim, device=w.device)
        for b in self.blocks:   # LayerScale folded into the frozen projections: gamma * (W x + b)
            g1, g2 = (b.ls1.gamma.float(), b.ls2.gamma.float()) if self.has_ls else (one, one)
            blocks.append(dict(qkv=b.attn.qkv.weight.to(BF16).contiguous(), qkv_b=b.attn.qkv.bias.float().contiguous(),
                               proj=(g1[:, None] * b.attn.proj.weight.float()).to(BF16).contiguous(), proj_b=(g1 * b.attn.proj.bias.float()).contiguous(),
                               fc1=b.mlp.fc1.weight.to(BF16).contiguous(), fc1_b=b.mlp.fc1.bias.float().contiguous(),
                               fc2=(g2[:, None] * b.mlp.fc2.weight.float()).to(BF16).contiguous(), fc2_b=(g2 * b.mlp.fc2.bias.float()).contiguous()))
        rt["blocks"] = blocks
        self._rt = rt

    @torch.no_grad()
    def patch_tokens(self, frames_u8: torch.Tensor, mean=DINO_RGB_MEANS, std=DINO_RGB_STDS, crop_x: int = 3) -> torch.Tensor:
        """frames_u8 [B,H,W,3] uint8 -> normed tokens [B, (1 +) gh*gw, dim] bf16 (class token first when the geometry has one).
        The patch grid is (H // patch) x ((W - 2 crop_x) // patch): 224 x 384 -> 16 x 27 (DINOv2), 256 x 256 -> 16 x 16 (SigLIP)."""
        B, H, W, _ = frames_u8.shape
        gh, gw = H // self.patch, (W - 2 * crop_x) // self.patch
        if self._rt is None or (self._rt["gh"], self._rt["gw"]) != (gh, gw):
            self.sync(gh, gw)
        rt = self._rt
        KP, C = rt["KP"], self.dim
        nc = 1 if self.has_cls else 0
        NP, S = gh * gw, gh * gw + nc
        dev = frames_u8.device
        cols = torch.empty(B * NP, KP, device=dev, dtype=BF16)
        ops.patchify_u8(frames_u8.contiguous(), mean, std, cols, crop_x=crop_x, P=self.patch, gh=gh, gw=gw)
        pt = ops.gemm_nt(cols, rt["pe_w"], B * NP, C, KP, bias=rt["pe_b"])
        # token rows padded to a whole number of 256-row GEMM panels (128 frames x 433 tokens = 216.5 panels): the pad rows are zeros at the input and are
        # carried through the row-wise kernels (LayerNorm, GEMMs) like any other row -- attention works per frame and never reads them -- so that no GEMM of
        # the trunk ends in a ragged tail (round 5: the 128-row tail launches behind the assembly GEMMs were 6.5 % of the ViT's kernel time)
        n_real = B * S
        n = (n_real + 255) // 256 * 256
        x = torch.empty(n, C, device=dev, dtype=BF16)
        if n > n_real:
            x[n_real:].zero_()
        ops.vit_tokens(pt, rt["cls"], rt["pos"], B, NP, C, x)
        ao = torch.empty(n, C, device=dev, dtype=BF16)      # attention output, reused by every block (attention writes the B * S real rows)
        if n > n_real:
            ao[n_real:].zero_()
        for b, w in zip(self.blocks, rt["blocks"]):
            h, _, _ = ops.norm_fwd(x, b.norm1.weight, b.norm1.bias, 1e-6, n, D=C, save_stats=False)
            qkv = ops.gemm_nt(h, w["qkv"], n, 3 * C, C, bias=w["qkv_b"])
            ops.attn_fwd(qkv, qkv[:, C:], qkv[:, 2 * C:], 3 * C, B, S, self.heads, 0.125, save_lse=False, out=ao)
            x = ops.gemm_nt(ao, w["proj"], n, C, C, bias=w["proj_b"], residual=x)
            h, _, _ = ops.norm_fwd(x, b.norm2.weight, b.norm2.bias, 1e-6, n, D=C, save_stats=False)
            f = ops.gemm_nt(h, w["fc1"], n, 4 * C, C, bias=w["fc1_b"], act=ops.ACT_GELU)
            x = ops.gemm_nt(f, w["fc2"], n, C, 4 * C, bias=w["fc2_b"], residual=x)
        out, _, _ = ops.norm_fwd(x, self.norm.weight, self.norm.bias, 1e-6, n_real, D=C, save_stats=False)
        return out[:n_real].view(B, S, C)


class _ViTPreprocessorBase:
    """Raw uint8 frames -> frozen ViT -> AdaptiveAvgPool2d((7, 12)).  ``process`` returns the reference's fp32 (B, C, 7, 12);
    ``process_tokens`` writes the storage-native bf16 tokens [B, ncam, 84, C]."""
    MEAN, STD, CROP_X, HW = DINO_RGB_MEANS, DINO_RGB_STDS, 3, (224, 384)

    def _setup(self, rgb_input_uuid, output_uuid, model_type, device, flatten, augmenter=None):
        self.input_uuids, self.uuid, self.device = [rgb_input_uuid], output_uuid, torch.device(device)
        # optional frame augmentation in front of the patchify kernel: a DataAugmentationPreprocessor(use_augmentation=True) (anything with ``augment_u8``), or
        # one per camera (a list) for process_tokens / process_tokens_all_cameras.  None: the frames go to the trunk as they come.
        self.augmenters = [] if augmenter is None else (list(augmenter) if isinstance(augmenter, (list, tuple)) else [augmenter])
        self.vit = DinoViT(self.device, **VIT_PRESETS[model_type])
        C = self.vit.dim
        self.observation_space = Box(-float("inf"), float("inf"), (7 * 12, C) if flatten else (7, 12, C))

    def to(self, device):
        return self

    def _tokens(self, fr):
        assert tuple(fr.shape[1:3]) == self.HW, f"Expected shape is {self.HW[0]}x{self.HW[1]}; got {tuple(fr.shape[1:3])}"
        return self.vit.patch_tokens(fr, self.MEAN, self.STD, crop_x=self.CROP_X)

    def _augment(self, fr, cam: int = 0):
        if not self.augmenters:
            return fr
        assert cam < len(self.augmenters) or len(self.augmenters) == 1, f"camera {cam}: {len(self.augmenters)} augmenters"
        return self.augmenters[cam if len(self.augmenters) > 1 else 0].augment_u8(fr)

    @torch.no_grad()
    def process(self, obs: Dict[str, torch.Tensor], *a, **k) -> torch.Tensor:
        assert len(self.augmenters) <= 1, "process serves one camera: pass one augmenter"
        fr = self._augment(obs[self.input_uuids[0]].to(self.device))
        x = self._tokens(fr)
        B, v = fr.shape[0], self.vit
        gh, gw = self._rt_grid()
        out = torch.empty(B, v.dim, 7, 12, device=self.device, dtype=torch.float32)
        ops.adaptive_pool_tokens(x, B, 1 if v.has_cls else 0, gh, gw, v.dim, 7, 12, chw_out=out)
        return out

    def _rt_grid(self):
        return self.vit._rt["gh"], self.vit._rt["gw"]

    @torch.no_grad()
    def process_tokens(self, frames_u8: torch.Tensor, out_tokens: torch.Tensor, cam: int, ncam: int = 2):
        x = self._tokens(self._augment(frames_u8.to(self.device), cam))
        gh, gw = self._rt_grid()
        ops.adaptive_pool_tokens(x, frames_u8.shape[0], 1 if self.vit.has_cls else 0, gh, gw, self.vit.dim, 7, 12, cam=cam, ncam=ncam, tok_out=out_tokens)


    @torch.no_grad()
    def process_tokens_all_cameras(self, frames_u8: torch.Tensor, out_tokens: torch.Tensor):
        """frames_u8 [ncam * B, H, W, 3] (camera-major: all envs' frames of camera 0, then camera 1, ...) -> out_tokens [B, ncam, 84, C] in ONE pass of the trunk
        (the rollout's two cameras share the frozen encoder: one 2B-frame batch fills the GPU better than two B-frame batches).  With augmenters (one per
        camera) each camera's slice is augmented by its own augmenter first."""
        B, ncam = out_tokens.shape[0], out_tokens.shape[1]
        assert frames_u8.shape[0] == ncam * B
        fr = frames_u8.to(self.device)
        if self.augmenters:
            assert len(self.augmenters) == ncam, f"{ncam} cameras need {ncam} augmenters, got {len(self.augmenters)}"
            # an augmenter that resizes (SigLIPDataAugmentationPreprocessor) names its output size in ``size``: both cameras' resized frames share one buffer
            oh, ow = getattr(self.augmenters[0], "size", None) or fr.shape[1:3]
            aug = torch.empty(fr.shape[0], oh, ow, 3, device=fr.device, dtype=fr.dtype)
            for cam, a in enumerate(self.augmenters):
                a.augment_u8(fr[cam * B:(cam + 1) * B], out=aug[cam * B:(cam + 1) * B])
            fr = aug
        x = self._tokens(fr)
        gh, gw = self._rt_grid()
        for cam in range(ncam):
            ops.adaptive_pool_tokens(x[cam * B:(cam + 1) * B], B, 1 if self.vit.has_cls else 0, gh, gw, self.vit.dim, 7, 12, cam=cam, ncam=ncam, tok_out=out_tokens)


class DinoViTPreprocessor(_ViTPreprocessorBase):
    """dino_preprocessors.py:38-125: 224 x 384 frames, W crop [3:-3], DINOv2 ``x_norm_patchtokens`` -> (B, C, 16, 27) -> pool (7, 12)."""

    def __init__(self, rgb_input_uuid: str, output_uuid: str, dino_model_type: str = "dinov2_vits14", device="cuda", flatten: bool = True, augmenter=None, **kw):
        if dino_model_type == "dinov2_vitg14":
            raise NotImplementedError("dinov2_vitg14 (SwiGLU-fused MLP, 40 blocks) is not built; ViT-S/B/L-14 are")
        assert dino_model_type in ("dinov2_vits14", "dinov2_vitb14", "dinov2_vitl14"), dino_model_type
        self._setup(rgb_input_uuid, output_uuid, dino_model_type, device, flatten, augmenter)


class SigLIPPreprocessor(_ViTPreprocessorBase):
    """siglip_preprocessors.py:18-104: 256 x 256 frames, mean = std = 0.5, timm trunk ``forward_features`` (B, 256, 768) ->
    (B, 768, 16, 16) -> AdaptiveAvgPool2d((7, 12)).  Weights come from open_clip's hub download in the reference: random-init geometry
    here (parity pinned against the fp32 restatement of the published timm forward, oracle/ref_vit.py)."""
    SIGLIP_RGB_MEANS, SIGLIP_RGB_STDS = (0.5, 0.5, 0.5), (0.5, 0.5, 0.5)
    MEAN, STD, CROP_X, HW = SIGLIP_RGB_MEANS, SIGLIP_RGB_STDS, 0, (256, 256)

    def __init__(self, rgb_input_uuid: str, output_uuid: str, siglip_model_type: str = "ViT-B-16-SigLIP-256", device="cuda", flatten: bool = True, augmenter=None, **kw):
        assert siglip_model_type in ("ViT-B-16-SigLIP-256", "ViT-L-16-SigLIP-256"), siglip_model_type
        self._setup(rgb_input_uuid, output_uuid, siglip_model_type, device, flatten, augmenter)


# ---- CLIP RN50 conv trunk (clip_resnet_50_3) ----------------------------------------------------------------------------------------------
CLIP_RGB_MEANS, CLIP_RGB_STDS = DINO_RGB_MEANS, DINO_RGB_STDS      # preprocessors.py:27 -- the DINO constants above ARE the CLIP mean / std
BN_EPS = 1e-5


class _FoldedConv(NamedTuple):
    """one folded convolution as the kernels take it: w bf16 [Cout, taps, Cin], b fp32 [Cout]"""
    w: torch.Tensor
    b: torch.Tensor
    cin: int
    cout: int
    taps: int


class ClipResNet(nn.Module):
    """Frozen CLIP ``ModifiedResNet`` trunk without its attention pool (image_encoders.py:11-48: ``ClipResNet``, ``pool=False``), under the parameter names of CLIP's
    ``visual`` module: ``conv1.weight``, ``bn1.{weight,bias,running_mean,running_var}``, ..., ``layer2.0.downsample.0.weight``, ``layer2.0.downsample.1.running_var``.
    The ``clip`` package is third-party and not in the reference tree; its published forward is restated:

      stem   conv1 3->w/2 3x3 stride 2, conv2 w/2->w/2 3x3, conv3 w/2->w 3x3 (each: no bias, BatchNorm, ReLU), AvgPool2d(2)
      block  conv1 1x1 -> planes, conv2 3x3 (stride 1) -> planes (each BN + ReLU), AvgPool2d(stride) if stride > 1, conv3 1x1 -> 4 planes + BN;
             identity = downsample (AvgPool2d(stride), 1x1 conv, BN) in the first block of every stage; out = ReLU(conv3 path + identity)
      stages planes w, 2w, 4w, 8w with strides 1, 2, 2, 2 and ``layers`` blocks; output 32 w channels at 1/32 of the frame: (2048, 7, 12) at 224 x 384.

    Random-init geometry (CLIP's weights are a download); ``load_state_dict`` takes a CLIP ``visual.*`` state dict with the prefix stripped (``attnpool.*`` and
    ``num_batches_tracked`` entries are ignored).  ``sync()`` folds every eval-mode BatchNorm into its convolution and re-lays the weights for the kernels;
    ``forward`` is then a chain of launches on NHWC bf16 rows: the fused u8 stem, the implicit-GEMM convolution (csrc/conv.hip) for every 3x3, the narrow 1x1 and the
    residual + ReLU 1x1, the bf16 NT GEMM for the other 1x1 convolutions."""
    CHUNK = 16      # frames per pass: the largest activation (layer1's output, H/4 x W/4 x 256 bf16) is 2.75 MB per 224 x 384 frame

    def __init__(self, device, width: int = 64, layers=(3, 4, 6, 3)):
        super().__init__()
        assert width % 64 == 0, "channel counts must be multiples of 32"
        d = torch.device(device)
        self.width, self.layers = width, tuple(layers)

        def conv(cout, cin, k, gain=1.0):      # He initialisation; the residual branches end small (gain 0.25) so that 16 blocks do not blow the scale up
            m = _NS()
            m.weight = nn.Parameter((torch.randn(cout, cin, k, k) * (gain * math.sqrt(2.0 / (cin * k * k)))).to(d), requires_grad=False)
            return m

        def bn(c):
            m = _NS()
            m.weight = nn.Parameter(torch.ones(c, device=d), requires_grad=False)
            m.bias = nn.Parameter(torch.zeros(c, device=d), requires_grad=False)
            m.register_buffer("running_mean", torch.zeros(c, device=d))
            m.register_buffer("running_var", torch.ones(c, device=d))
            return m

        self.conv1, self.bn1 = conv(width // 2, 3, 3), bn(width // 2)
        self.conv2, self.bn2 = conv(width // 2, width // 2, 3), bn(width // 2)
        self.conv3, self.bn3 = conv(width, width // 2, 3), bn(width)
        inplanes = width
        for i, n in enumerate(self.layers):
            planes, stride = width << i, (1 if i == 0 else 2)
            blocks = []
            for j in range(n):
                b = _NS()
                b.stride = stride if j == 0 else 1
                b.conv1, b.bn1 = conv(planes, inplanes, 1), bn(planes)
                b.conv2, b.bn2 = conv(planes, planes, 3), bn(planes)
                b.conv3, b.bn3 = conv(4 * planes, planes, 1, gain=0.25), bn(4 * planes)
                if b.stride > 1 or inplanes != 4 * planes:
                    b.downsample = _NS()          # keys "-1" (the pool: no parameters), "0", "1" of CLIP's Sequential
                    b.downsample.add_module("0", conv(4 * planes, inplanes, 1))
                    b.downsample.add_module("1", bn(4 * planes))
                inplanes = 4 * planes
                blocks.append(b)
            setattr(self, f"layer{i + 1}", nn.Sequential(*blocks))
        self.out_channels = inplanes
        self._rt = None

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        sd = {k: v for k, v in state_dict.items() if not k.startswith("attnpool.") and not k.endswith("num_batches_tracked")}
        self._rt = None
        return super().load_state_dict(sd, strict=strict, **kw)

    @staticmethod
    def fold(conv, bn):
        """(w * gamma / sqrt(var + eps), beta - mean * gamma / sqrt(var + eps)) in fp32"""
        s = bn.weight.float() / torch.sqrt(bn.running_var.float() + BN_EPS)
        return conv.weight.float() * s[:, None, None, None], bn.bias.float() - bn.running_mean.float() * s

    def sync(self):
        def lay(conv, bn):      # [Cout, Cin, kh, kw] -> K-major [Cout, taps, Cin] bf16 + fp32 bias
            w, b = self.fold(conv, bn)
            co, ci, kh, kw = w.shape
            return _FoldedConv(w.permute(0, 2, 3, 1).reshape(co, kh * kw, ci).to(BF16).contiguous(), b.contiguous(), ci, co, kh * kw)

        rt = {}
        w, b = self.fold(self.conv1, self.bn1)      # stem: fp32 [27, Cout] holding the bf16-rounded folded weights (every folded weight of the trunk is a bf16 value)
        rt["stem"] = (w.to(BF16).float().permute(2, 3, 1, 0).reshape(27, -1).contiguous(), b.contiguous())
        rt["conv2"], rt["conv3"] = lay(self.conv2, self.bn2), lay(self.conv3, self.bn3)
        rt["blocks"] = []
        for i in range(len(self.layers)):
            for blk in getattr(self, f"layer{i + 1}"):
                down = lay(getattr(blk.downsample, "0"), getattr(blk.downsample, "1")) if hasattr(blk, "downsample") else None
                rt["blocks"].append((blk.stride, lay(blk.conv1, blk.bn1), lay(blk.conv2, blk.bn2), lay(blk.conv3, blk.bn3), down))
        self._rt = rt

    @staticmethod
    def _conv1x1(x, L, B, H, W, relu: bool):
        M = B * H * W
        if L.cout % 128 == 0 and L.cin % 64 == 0:      # the bf16 NT GEMM's shapes; the two 64-wide 1x1 of layer1 stay on the convolution kernel
            return ops.gemm_nt(x.view(M, L.cin), L.w.view(L.cout, L.cin), M, L.cout, L.cin, bias=L.b, act=ops.ACT_RELU if relu else ops.ACT_NONE)
        return ops.conv_nhwc(x, L.w, L.b, B, H, W, 1, ops.EPI_RELU if relu else ops.EPI_BIAS)

    def _chunk(self, fr, mean, std, out, y_group, y_group_stride):
        rt = self._rt
        B, H, W, _ = fr.shape
        assert rt["stem"][0].shape[1] == 32, "the fused stem kernel is built for CLIP RN50's 32 stem channels (width 64)"
        h = ops.conv_stem_u8(fr, mean, std, *rt["stem"])
        H, W = H // 2, W // 2
        h = ops.conv_nhwc(h, rt["conv2"].w, rt["conv2"].b, B, H, W, 9, ops.EPI_RELU)
        h = ops.conv_nhwc(h, rt["conv3"].w, rt["conv3"].b, B, H, W, 9, ops.EPI_RELU)
        h = ops.avgpool2_nhwc(h, B, H, W, rt["conv3"].cout)
        H, W = H // 2, W // 2
        last = len(rt["blocks"]) - 1
        for k, (stride, c1, c2, c3, down) in enumerate(rt["blocks"]):
            o = self._conv1x1(h, c1, B, H, W, True)
            o = ops.conv_nhwc(o, c2.w, c2.b, B, H, W, 9, ops.EPI_RELU)
            idn = h
            if stride > 1:
                o = ops.avgpool2_nhwc(o, B, H, W, c2.cout)
                idn = ops.avgpool2_nhwc(h, B, H, W, c1.cin)
                H, W = H // 2, W // 2
            if down is not None:
                idn = self._conv1x1(idn, down, B, H, W, False)
            if k == last:      # the trunk's output rows go where the caller wants them (dense rows, or one camera slot of the token tensor)
                ops.conv_nhwc(o, c3.w, c3.b, B, H, W, 1, ops.EPI_RES_RELU, residual=idn, out=out, ldy=c3.cout, y_group=y_group, y_group_stride=y_group_stride)
            else:
                h = ops.conv_nhwc(o, c3.w, c3.b, B, H, W, 1, ops.EPI_RES_RELU, residual=idn)

    @torch.no_grad()
    def forward(self, frames_u8: torch.Tensor, mean=CLIP_RGB_MEANS, std=CLIP_RGB_STDS, out: Optional[torch.Tensor] = None, cam: Optional[int] = None) -> torch.Tensor:
        """frames_u8 [B,H,W,3] uint8 (H, W multiples of 32) -> bf16 rows [B, H/32 * W/32, C]: a new tensor, or ``out``; with ``cam`` the rows of frame b are written
        into ``out[b, cam]`` of a token tensor [B, ncam, H/32 * W/32, C]."""
        B, H, W, _ = frames_u8.shape
        assert frames_u8.dtype == torch.uint8 and H % 32 == 0 and W % 32 == 0 and H > 0 and W > 0, f"uint8 frames with H, W multiples of 32; got {tuple(frames_u8.shape)}"
        if self._rt is None:
            self.sync()
        P, C = (H // 32) * (W // 32), self.out_channels
        if out is None:
            assert cam is None
            out = torch.empty(B, P, C, device=frames_u8.device, dtype=BF16)
        assert out.dtype == BF16 and out.is_contiguous() and out.shape[0] == B and tuple(out.shape[-2:]) == (P, C), tuple(out.shape)
        ncam = out.shape[1] if cam is not None else 1
        assert (cam or 0) < ncam
        fr = frames_u8.contiguous()
        for b0 in range(0, B, self.CHUNK):
            b1 = min(B, b0 + self.CHUNK)
            dst = out[b0:, cam] if cam is not None else out[b0:]
            self._chunk(fr[b0:b1], mean, std, dst, P if cam is not None else 0, ncam * P if cam is not None else 0)
        return out


class ClipResNetPreprocessor(_ViTPreprocessorBase):
    """image_encoders.py:11-48 + preprocessors.py:27: 224 x 384 uint8 frames -> CLIP normalisation -> frozen CLIP RN50 trunk -> (B, 2048, 7, 12).  Same surface as the
    ViT preprocessors: ``process`` returns the reference's fp32 (B, 2048, 7, 12), ``process_tokens`` / ``process_tokens_all_cameras`` write the storage-native bf16
    tokens [B, ncam, 84, 2048] -- the trunk's last block writes its rows straight into the camera slot."""
    MEAN, STD, HW = CLIP_RGB_MEANS, CLIP_RGB_STDS, (224, 384)

    def __init__(self, rgb_input_uuid: str, output_uuid: str, device="cuda", flatten: bool = True, augmenter=None, **kw):
        self.input_uuids, self.uuid, self.device = [rgb_input_uuid], output_uuid, torch.device(device)
        self.augmenters = [] if augmenter is None else (list(augmenter) if isinstance(augmenter, (list, tuple)) else [augmenter])
        self.resnet = ClipResNet(self.device)
        C = self.resnet.out_channels
        self.observation_space = Box(-float("inf"), float("inf"), (7 * 12, C) if flatten else (7, 12, C))

    def _check(self, fr):
        assert tuple(fr.shape[1:3]) == self.HW, f"Expected shape is {self.HW[0]}x{self.HW[1]}; got {tuple(fr.shape[1:3])}"
        return fr

    @torch.no_grad()
    def process(self, obs: Dict[str, torch.Tensor], *a, **k) -> torch.Tensor:
        assert len(self.augmenters) <= 1, "process serves one camera: pass one augmenter"
        fr = self._check(self._augment(obs[self.input_uuids[0]].to(self.device)))
        B, C = fr.shape[0], self.resnet.out_channels
        x = self.resnet(fr, self.MEAN, self.STD)
        out = torch.empty(B, C, 7, 12, device=self.device, dtype=torch.float32)
        ops.adaptive_pool_tokens(x, B, 0, 7, 12, C, 7, 12, chw_out=out)      # 7 x 12 -> 7 x 12: the token rows transposed to fp32 channels-first
        return out

    @torch.no_grad()
    def process_tokens(self, frames_u8: torch.Tensor, out_tokens: torch.Tensor, cam: int, ncam: int = 2):
        assert out_tokens.shape[1] == ncam
        self.resnet(self._check(self._augment(frames_u8.to(self.device), cam)), self.MEAN, self.STD, out=out_tokens, cam=cam)

    @torch.no_grad()
    def process_tokens_all_cameras(self, frames_u8: torch.Tensor, out_tokens: torch.Tensor):
        """frames_u8 [ncam * B, H, W, 3], camera-major -> out_tokens [B, ncam, 84, 2048]; with augmenters (one per camera) each camera's slice is augmented first"""
        B, ncam = out_tokens.shape[0], out_tokens.shape[1]
        assert frames_u8.shape[0] == ncam * B
        fr = self._check(frames_u8.to(self.device))
        if self.augmenters:
            assert len(self.augmenters) == ncam, f"{ncam} cameras need {ncam} augmenters, got {len(self.augmenters)}"
        for cam in range(ncam):
            x = fr[cam * B:(cam + 1) * B]
            self.resnet(self.augmenters[cam].augment_u8(x) if self.augmenters else x, self.MEAN, self.STD, out=out_tokens, cam=cam)
