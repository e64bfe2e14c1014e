#!/usr/bin/env python3
"""Cost of the sampled frame augmentation (csrc/augment.hip) at the rollout's size: 64 envs x 2 cameras of 224 x 384 uint8 frames.

  * per-launch time of the three augmentation kernels on one camera's 64 frames (HIP events around `--reps` back-to-back launches after warm-up);
  * the ViT preprocessor step (DinoViTPreprocessor.process_tokens_all_cameras on the 128 frames) without and, where the tree has them, with one augmenter per camera,
    alternating the two within the run; the host draws of a call (ColorJitter order, crop box) are part of the step;
  * a hash of the un-augmented step's output tokens, to compare two trees on the same frames.

Runs on a tree without the augmentation too (it then reports the plain step only): the same file times the parent commit.  Results: profiles/augment_ab.txt;
against the parent of the change that gave both launch forms one body per stage: profiles/augment_shared_ab.txt."""
import argparse
import hashlib
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from safevla_amd import ops
from safevla_amd.preproc import DataAugmentationPreprocessor, DinoViTPreprocessor


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev, B = torch.device("cuda"), a.envs
    has_aug = hasattr(ops, "aug_gray_partials")
    g = torch.Generator().manual_seed(0)
    frames = torch.randint(0, 256, (2 * B, 224, 384, 3), generator=g, dtype=torch.uint8).to(dev)
    torch.manual_seed(0)
    plain = DinoViTPreprocessor("rgb", "rgb_dinov2", device=dev)
    tok = torch.zeros(B, 2, 84, 384, device=dev, dtype=torch.bfloat16)
    plain.process_tokens_all_cameras(frames, tok)
    torch.cuda.synchronize()
    print(f"un-augmented tokens sha256 {hashlib.sha256(tok.view(torch.int16).cpu().numpy().tobytes()).hexdigest()[:16]}")
    mb = frames[:B].numel() / 1e6
    if has_aug:
        from safevla_amd.preproc import AugmentCall, gaussian_weights, sample_augment_params
        random.seed(0)
        p = sample_augment_params()._replace(posterize_draws=(1, 0, 0, 0), sharpness=1)
        order = [0, 2, 3, 1]                                   # contrast last: the gray reduction applies the three operations before it
        f = [p.factor(o) for o in order]
        x = frames[:B].contiguous()
        part = ops.aug_gray_partials(x, order[:3], f[:3])
        y, z = torch.empty_like(x), torch.empty_like(x)
        wx, wy = gaussian_weights(5, p.sigma), gaussian_weights(9, p.sigma)
        box = (0, 42, 224, 299)
        t = timed(lambda: ops.aug_gray_partials(x, order[:3], f[:3]), a.reps)
        print(f"aug_gray_partials_kernel      {B} frames: {t * 1e3:8.1f} us per launch  ({mb / t:7.1f} GB/s of frame bytes read)")
        t = timed(lambda: ops.aug_jitter_blur(x, order, f, part, wx, wy, out=y), a.reps)
        print(f"aug_jitter_blur_kernel        {B} frames: {t * 1e3:8.1f} us per launch  ({2 * mb / t:7.1f} GB/s read + written)")
        t = timed(lambda: ops.aug_resize_post_sharp(y, box, True, True, out=z), a.reps)
        print(f"aug_resize_post_sharp_kernel  {B} frames: {t * 1e3:8.1f} us per launch  ({2 * mb / t:7.1f} GB/s read + written)")
        torch.manual_seed(0)
        augd = DinoViTPreprocessor("rgb", "rgb_dinov2", device=dev, augmenter=[
            DataAugmentationPreprocessor("rgb", "a0", device=dev, use_augmentation=True, generator=torch.Generator().manual_seed(1)),
            DataAugmentationPreprocessor("manip", "a1", device=dev, use_augmentation=True, generator=torch.Generator().manual_seed(2))])
        tok2 = torch.zeros_like(tok)
    for r in range(a.rounds):                                  # alternate the two within the run
        t_plain = timed(lambda: plain.process_tokens_all_cameras(frames, tok), max(5, a.reps // 5))
        line = f"round {r}: ViT step {2 * B} frames, no augmenter {t_plain:7.3f} ms ({2 * B / t_plain:6.1f} k frames/s)"
        if has_aug:
            t_aug = timed(lambda: augd.process_tokens_all_cameras(frames, tok2), max(5, a.reps // 5))
            line += f" | two augmenters {t_aug:7.3f} ms (+{t_aug - t_plain:6.3f} ms, +{100 * (t_aug - t_plain) / t_plain:4.1f} %)"
        print(line)


if __name__ == "__main__":
    main()
