#!/usr/bin/env python3
"""Cost of the antialiased bicubic u8 resize (csrc/resize.hip) at the SigLIP presets' geometry, 224 x 384 -> 256 x 256, against the stock route on the same GPU:
F.interpolate(x.permute(0, 3, 1, 2).float(), antialias=True) -> clamp -> round -> uint8 -> permute back.

HIP events around `--reps` back-to-back calls after `--warmup` calls, on 128 frames (two cameras of 64 environments) and on 2 frames (one agent step); the two
routes alternate within the run.  The kernel's algorithmic bytes (frames read once + frames written once) over its time is reported as a fraction of the HBM
peak (8.0 TB/s).  Also prints how far the two routes' outputs differ.  Results: profiles/resize_ab.txt."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from safevla_amd import ops

HBM_PEAK = 8.0e12


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps * 1e-3      # seconds per call


def stock(x, hw):
    y = F.interpolate(x.permute(0, 3, 1, 2).float(), size=hw, mode="bicubic", antialias=True, align_corners=False)
    return y.clamp(0, 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev, hw = torch.device("cuda"), (256, 256)
    for B in (128, 2):
        x = torch.randint(0, 256, (B, 224, 384, 3), generator=torch.Generator().manual_seed(B), dtype=torch.uint8).to(dev)
        out = torch.empty(B, *hw, 3, dtype=torch.uint8, device=dev)
        d = (ops.resize_bicubic_aa_u8(x, hw, out=out).int() - stock(x, hw).int()).abs()
        print(f"{B} frames 224x384 -> 256x256: kernel vs stock route: {int((d > 0).sum())} of {d.numel()} values differ, by at most {int(d.max())}")
        nbytes = x.numel() + out.numel()
        for r in range(a.rounds):
            tk = timed(lambda: ops.resize_bicubic_aa_u8(x, hw, out=out), a.reps, a.warmup)
            ts = timed(lambda: stock(x, hw), a.reps, a.warmup)
            print(f"  round {r}: kernel {tk * 1e6:8.1f} us ({nbytes / tk / 1e12:5.2f} TB/s = {nbytes / tk / HBM_PEAK:5.3f} of the HBM peak) | stock route {ts * 1e6:8.1f} us | "
                  f"stock / kernel {ts / tk:5.1f} x")


if __name__ == "__main__":
    main()
