#!/usr/bin/env python3
"""Cost of the per-trajectory random frame augmentation (the grouped kernels of csrc/augment.hip) against the only route without it: one application of the
single-transform launches (same file, same device bodies) per trajectory, on that trajectory's slice of the batch.

  * leg A: G x preproc.apply_augment_u8 on the G slices (3 G launches, G host conversions); leg B: one preproc.apply_random_augment_u8 (3 launches, each with its
    108-byte-per-group table upload) -- at 16 trajectories x 8 frames of 224 x 384 (the camera) and of 256 x 256 (the SigLIP presets' input);
  * G = 1 at 64 frames: the grouped form against preproc.apply_augment_u8 on the same transform -- the extra work is one table read per block and the three uploads;
  * per-kernel time of the three grouped launches at G = 16 (each with its table upload), and at G = 1 each single-transform kernel against its grouped twin.

HIP events around `--reps` back-to-back applications after warm-up, the two legs alternated within one run, `--rounds` times; the host work of a leg (building the
table, argument conversion) is inside its window.  Both legs write into preallocated outputs; their results are compared bit for bit before anything is timed.
Results: profiles/augment_grouped_ab.txt; against the parent of the change that gave both forms one body per stage: profiles/augment_shared_ab.txt."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from safevla_amd import ops
from safevla_amd.preproc import apply_augment_u8, apply_random_augment_u8, gaussian_weights, sample_random_augment_call


def timed(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps * 1e3      # us


def draws(G, H, W, seed):
    """G calls of the sampler with the posterize mask folded to what the single-transform path can express (0xFE or none), so that both legs apply the same transforms"""
    g = torch.Generator().manual_seed(seed)
    calls = [sample_random_augment_call(H, W, g) for _ in range(G)]
    return [c._replace(post_mask=0xFF if c.post_mask == 0xFF else 0xFE) for c in calls]


def ab(G, L, H, W, reps, rounds, seed):
    x = torch.randint(0, 256, (G * L, H, W, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8).cuda()
    calls = draws(G, H, W, seed)
    single = [c.as_augment_call() for c in calls]
    ya, yb = torch.empty_like(x), torch.empty_like(x)
    slices = [(x[k * L:(k + 1) * L], ya[k * L:(k + 1) * L]) for k in range(G)]

    def leg_a():
        for (xs, ys), c in zip(slices, single):
            apply_augment_u8(xs, c, out=ys)

    def leg_b():
        apply_random_augment_u8(x, calls, L, out=yb)

    leg_a(); leg_b()
    torch.cuda.synchronize()
    assert torch.equal(ya, yb), "the two legs differ"
    rows = []
    for r in range(rounds):
        ta, tb = timed(leg_a, reps), timed(leg_b, reps)
        rows.append((ta, tb))
        print(f"  round {r}: A {G:2d} x single-transform {ta:8.1f} us | B grouped {tb:8.1f} us | B / A {tb / ta:5.3f}")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    verdicts = []
    for H, W in ((224, 384), (256, 256)):
        print(f"16 trajectories x 8 frames of {H} x {W} ({16 * 8 * H * W * 3 / 1e6:.1f} MB of frames), outputs bit-equal:")
        rows = ab(16, 8, H, W, a.reps, a.rounds, seed=H)
        worst = max(tb / ta for ta, tb in rows)
        verdicts.append((f"B no slower than A at G = 16, {H} x {W}", worst <= 1.0, f"worst round B / A = {worst:.3f}"))
    for H, W in ((224, 384), (256, 256)):
        print(f"G = 1, 64 frames of {H} x {W}, outputs bit-equal:")
        rows = ab(1, 64, H, W, a.reps, a.rounds, seed=H + 1)
        worst = max(tb / ta for ta, tb in rows)
        verdicts.append((f"G = 1 grouped within 10 % of the single-transform launches, {H} x {W}", worst <= 1.10, f"worst round B / A = {worst:.3f}"))
    # per kernel, G = 16, camera size
    G, L, H, W = 16, 8, 224, 384
    x = torch.randint(0, 256, (G * L, H, W, 3), generator=torch.Generator().manual_seed(3), dtype=torch.uint8).cuda()
    calls = draws(G, H, W, 3)
    table = ops.AugTable([(c.order, [c.factor(o) for o in c.order], gaussian_weights(5, c.sigma), gaussian_weights(9, c.sigma), c.box, c.post_mask, c.sharpen)
                          for c in calls], x.device)
    part = ops.aug_gray_partials_grouped(x, table, L)
    y, z = torch.empty_like(x), torch.empty_like(x)
    mb = x.numel() / 1e6
    print(f"per launch, G = 16 x 8 frames of {H} x {W} (table upload included):")
    t = timed(lambda: ops.aug_gray_partials_grouped(x, table, L), a.reps)
    print(f"  aug_gray_partials_grouped_kernel      {t:8.1f} us  ({mb / t * 1e3:7.1f} GB/s of frame bytes read)")
    t = timed(lambda: ops.aug_jitter_blur_grouped(x, table, L, part, out=y), a.reps)
    print(f"  aug_jitter_blur_grouped_kernel        {t:8.1f} us  ({2 * mb / t * 1e3:7.1f} GB/s read + written)")
    t = timed(lambda: ops.aug_resize_post_sharp_grouped(y, table, L, out=z), a.reps)
    print(f"  aug_resize_post_sharp_grouped_kernel  {t:8.1f} us  ({2 * mb / t * 1e3:7.1f} GB/s read + written)")
    # per kernel, G = 1: the single-transform kernel against its grouped twin on the same 64 frames and the same transform, alternated
    L, c = 64, draws(1, H, W, 4)[0]
    x = torch.randint(0, 256, (L, H, W, 3), generator=torch.Generator().manual_seed(4), dtype=torch.uint8).cuda()
    order, f = list(c.order), [c.factor(o) for o in c.order]
    k = order.index(ops.AUG_CONTRAST)
    wx, wy = gaussian_weights(5, c.sigma), gaussian_weights(9, c.sigma)
    table = ops.AugTable([(order, f, wx, wy, c.box, c.post_mask, c.sharpen)], x.device)
    part = ops.aug_gray_partials_grouped(x, table, L)
    y, z = torch.empty_like(x), torch.empty_like(x)
    pairs = [("gray partials", lambda: ops.aug_gray_partials(x, order[:k], f[:k]), lambda: ops.aug_gray_partials_grouped(x, table, L)),
             ("jitter + blur", lambda: ops.aug_jitter_blur(x, order, f, part, wx, wy, out=y), lambda: ops.aug_jitter_blur_grouped(x, table, L, part, out=y)),
             ("resize + posterize + sharpness", lambda: ops.aug_resize_post_sharp(y, c.box, c.post_mask == 0xFE, c.sharpen, out=z),
              lambda: ops.aug_resize_post_sharp_grouped(y, table, L, out=z))]
    print(f"per launch, G = 1 x 64 frames of {H} x {W}, single-transform kernel | grouped kernel (alternated, {a.rounds} rounds):")
    for name, single, grouped in pairs:
        rows = [(timed(single, a.reps), timed(grouped, a.reps)) for _ in range(a.rounds)]
        print(f"  {name:32s}" + "  ".join(f"{ts:7.1f} | {tg:7.1f} us" for ts, tg in rows))
    print("expectations:")
    for what, held, fig in verdicts:
        print(f"  {'HELD    ' if held else 'NOT HELD'}  {what}: {fig}")


if __name__ == "__main__":
    main()
