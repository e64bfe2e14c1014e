#!/usr/bin/env python3
"""Throughput of the frozen CLIP RN50 trunk (preproc.ClipResNet on csrc/conv.hip) at the rollout's size -- 2 cameras x 64 envs of 224 x 384 uint8 frames -- against
stock PyTorch-ROCm in the same run: torch.nn.functional.conv2d on bf16 channels_last tensors with the SAME folded weights (normalise, conv + bias, ReLU, avg_pool2d,
residual add), in the same chunks of frames.

  * frames/s of both legs, alternating them within the run: HIP events around `--reps` back-to-back passes after warm-up passes of every shape;
  * the distance between the two legs' outputs (same folded bf16 weights: summation order and the stock leg's own layer roundings);
  * the clock state as the SMI tool reports it before and after (read only).

`--leg ours|stock --reps 1 --rounds 1` runs one leg alone: the pass to wrap in `rocprofv3 --kernel-trace --stats` (a run of its own).  Results: profiles/clip_rn50_ab.txt."""
import argparse
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from safevla_amd.preproc import CLIP_RGB_MEANS, CLIP_RGB_STDS, ClipResNet

BF16 = torch.bfloat16


def timed(fn, reps, warmup=2):
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


class StockTrunk:
    """the same network on torch.nn.functional, bf16, channels_last, folded weights of ``m`` (every activation is a bf16 tensor, as in the HIP leg)"""

    def __init__(self, m: ClipResNet):
        cl = lambda w: w.to(BF16).contiguous(memory_format=torch.channels_last)
        f = lambda c, b: (lambda w, s: (cl(w), s.to(BF16)))(*m.fold(c, b))
        self.stem = [f(m.conv1, m.bn1), f(m.conv2, m.bn2), f(m.conv3, m.bn3)]
        self.blocks = []
        for i in range(len(m.layers)):
            for blk in getattr(m, f"layer{i + 1}"):
                down = f(getattr(blk.downsample, "0"), getattr(blk.downsample, "1")) if hasattr(blk, "downsample") else None
                self.blocks.append((blk.stride, f(blk.conv1, blk.bn1), f(blk.conv2, blk.bn2), f(blk.conv3, blk.bn3), down))
        dev = m.conv1.weight.device
        self.mean = torch.tensor(CLIP_RGB_MEANS, device=dev).view(1, 3, 1, 1)
        self.std = torch.tensor(CLIP_RGB_STDS, device=dev).view(1, 3, 1, 1)

    @torch.no_grad()
    def __call__(self, frames_u8, chunk):
        outs = []
        for b0 in range(0, frames_u8.shape[0], chunk):
            x = frames_u8[b0:b0 + chunk].permute(0, 3, 1, 2).float() / 255.0          # NHWC memory viewed as NCHW = channels_last
            x = ((x - self.mean) / self.std).to(BF16).contiguous(memory_format=torch.channels_last)
            x = F.relu(F.conv2d(x, *self.stem[0], stride=2, padding=1))
            x = F.relu(F.conv2d(x, *self.stem[1], padding=1))
            x = F.relu(F.conv2d(x, *self.stem[2], padding=1))
            x = F.avg_pool2d(x, 2)
            for stride, c1, c2, c3, down in self.blocks:
                o = F.relu(F.conv2d(x, *c1))
                o = F.relu(F.conv2d(o, *c2, padding=1))
                idn = x
                if stride > 1:
                    o, idn = F.avg_pool2d(o, 2), F.avg_pool2d(x, 2)
                if down is not None:
                    idn = F.conv2d(idn, *down)
                x = F.relu(F.conv2d(o, *c3) + idn)
            outs.append(x.permute(0, 2, 3, 1).reshape(x.shape[0], -1, x.shape[1]))
        return torch.cat(outs)


def clocks():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=60)
        keep = [ln.strip() for ln in r.stdout.splitlines() if "sclk" in ln or "mclk" in ln]
        return "; ".join(keep[:4]) or "(no clock lines)"
    except Exception as e:      # the tool is optional
        return f"(not read: {type(e).__name__})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--leg", choices=("both", "ours", "stock"), default="both")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    dev, n = torch.device("cuda"), 2 * a.envs
    g = torch.Generator().manual_seed(0)
    frames = torch.randint(0, 256, (n, 224, 384, 3), generator=g, dtype=torch.uint8).to(dev)
    torch.manual_seed(0)
    m = ClipResNet(dev)
    m.sync()
    stock = StockTrunk(m)
    ours = lambda: m(frames)
    theirs = lambda: stock(frames, m.CHUNK)
    print(f"{n} frames of 224 x 384 in chunks of {m.CHUNK}; {torch.cuda.get_device_name(0)}; clocks before: {clocks()}")
    if a.leg == "both":
        x, y = ours().float(), theirs().float()
        print(f"outputs: max |HIP - stock| / max |stock| = {float((x - y).abs().max() / y.abs().max()):.3e} (max |stock| {float(y.abs().max()):.2f})")
    for r in range(a.rounds):
        line = f"round {r}:"
        if a.leg in ("both", "ours"):
            t = timed(ours, a.reps)
            line += f"  HIP trunk {t:8.2f} ms per {n} frames ({n / t:6.2f} k frames/s)"
        if a.leg in ("both", "stock"):
            t = timed(theirs, a.reps)
            line += f"  | stock conv2d bf16 channels_last {t:8.2f} ms ({n / t:6.2f} k frames/s)"
        print(line, flush=True)
    print(f"clocks after: {clocks()}")


if __name__ == "__main__":
    main()
