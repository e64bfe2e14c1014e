#!/usr/bin/env python3
"""A/B of the long-sequence attention backward (csrc/attn_long.hip: head_dim 64, 256 < S <= 512) at decoder shapes rows x H x S:
  A  the only way to these gradients before: fp32 copies of the operands + the scalar fp32 kernels (what ``ops.attn_bwd`` still does for 96-wide heads above 256 keys);
  B  the shipped S = 256 backward on the same rows and heads, scaled by (S / 256)^2, the FLOP ratio -- how far the long kernels fall below that line is the figure of merit.
HIP-event timing, 20 timed repetitions after 5 warm-up calls, forward and backward, with a comparison of the bf16 and the fp32 gradients."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from safevla_amd import ops

H, HD = 8, 64
W = H * HD
SCALE = HD ** -0.5


def t_ms(fn, n=20, w=5):
    for _ in range(w): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def one(R, S, causal, fp32):
    """(forward ms, backward ms, gradients) of one route"""
    g = torch.Generator(device="cuda").manual_seed(R + S)
    qkv = (torch.randn(R * S, 3 * W, device="cuda", generator=g) * 0.5).to(torch.bfloat16)
    do = torch.randn(R * S, W, device="cuda", generator=g).to(torch.bfloat16)
    traj = (torch.arange(S, device="cuda")[None] // 131 + torch.zeros(R, 1, device="cuda", dtype=torch.long)).int().contiguous() if causal else None
    kw = dict(mask_mode=ops.MASK_BLOCK_CAUSAL if causal else ops.MASK_NONE, traj=traj)
    if fp32:      # the copies are part of the route: they are timed with it
        def fwd():
            q32 = qkv.float()
            return ops.attn_fwd(q32, q32[:, W:], q32[:, 2 * W:], 3 * W, R, S, H, SCALE, **kw)

        out, lse = fwd()
        dqkv = torch.zeros_like(qkv)

        def bwd():
            q32, o32, do32 = qkv.float(), out, do.float()
            d32 = torch.empty_like(q32)
            ops.attn_bwd(q32, q32[:, W:], q32[:, 2 * W:], 3 * W, o32, W, lse, do32, W, d32, d32[:, W:], d32[:, 2 * W:], 3 * W, R, S, H, SCALE, **kw)
            dqkv.copy_(d32)
    else:
        out, lse = ops.attn_fwd(qkv, qkv[:, W:], qkv[:, 2 * W:], 3 * W, R, S, H, SCALE, **kw)
        dqkv = torch.zeros_like(qkv)
        fwd = lambda: ops.attn_fwd(qkv, qkv[:, W:], qkv[:, 2 * W:], 3 * W, R, S, H, SCALE, out=out, **kw)
        bwd = lambda: ops.attn_bwd(qkv, qkv[:, W:], qkv[:, 2 * W:], 3 * W, out, W, lse, do, W, dqkv, dqkv[:, W:], dqkv[:, 2 * W:], 3 * W, R, S, H, SCALE, **kw)
    return t_ms(fwd), t_ms(bwd), dqkv.float()


for name, R, S, causal in [("decoder rows=64 S=320 block-causal", 64, 320, True), ("decoder rows=64 S=500 block-causal", 64, 500, True),
                           ("decoder rows=2  S=300 block-causal", 2, 300, True), ("no mask rows=64 S=500             ", 64, 500, False)]:
    f_new, b_new, g_new = one(R, S, causal, False)
    f_a, b_a, g_a = one(R, S, causal, True)
    f_256, b_256, _ = one(R, 256, causal, False)
    k = (S / 256.0) ** 2
    cos = torch.nn.functional.cosine_similarity(g_new.flatten(), g_a.flatten(), dim=0).item()
    print(f"{name}: forward  bf16 {f_new:.3f} ms | A fp32 route {f_a:.3f} ms ({f_a / f_new:.1f}x) | B S=256 {f_256:.3f} ms x {k:.2f} = {f_256 * k:.3f} ms (long / B = {f_new / (f_256 * k):.2f})")
    print(f"{' ' * len(name)}  backward bf16 {b_new:.3f} ms | A fp32 route {b_a:.3f} ms ({b_a / b_new:.1f}x) | B S=256 {b_256:.3f} ms x {k:.2f} = {b_256 * k:.3f} ms (long / B = {b_new / (b_256 * k):.2f})"
          f" | gradient cosine bf16 vs fp32 {cos:.6f}")
