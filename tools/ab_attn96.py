#!/usr/bin/env python3
"""A/B of the 96-wide attention (csrc/attn_hd96.hip) at the shapes of base_6 / siglip_base_3_6: the MFMA kernels against the fp32 detour (SVLA_ATTN96_F32=1: fp32 copies
of the operands + the scalar fp32 kernels, what these presets ran on before) and, for scale, against the 64-wide kernels at equal rows * H * S (2/3 of the FLOPs and bytes).
HIP-event timing, 20 timed repetitions after 5 warm-up calls, forward and backward, with a result comparison of the two 96-wide routes."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from safevla_amd import ops

H = 8


def t_ms(fn, n=20, w=5):
    for _ in range(w): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def one(R, S, hd, causal, p, detour):
    """(forward ms, backward ms, output, gradients) of one route"""
    os.environ["SVLA_ATTN96_F32"] = "1" if detour else "0"
    W = H * hd
    g = torch.Generator(device="cuda").manual_seed(R + S)
    qkv = (torch.randn(R * S, 3 * W, device="cuda", generator=g) * 0.5).to(torch.bfloat16)
    traj = (torch.arange(S, device="cuda")[None] // 17 + torch.zeros(R, 1, device="cuda", dtype=torch.long)).int().contiguous() if causal else None
    kw = dict(head_dim=hd, drop=ops.Dropout(77, 3, p) if p else None, mask_mode=ops.MASK_BLOCK_CAUSAL if causal else ops.MASK_NONE, traj=traj)
    out, lse = ops.attn_fwd(qkv, qkv[:, W:], qkv[:, 2 * W:], 3 * W, R, S, H, hd ** -0.5, **kw)
    do = (torch.randn(R * S, W, device="cuda", generator=g)).to(torch.bfloat16)
    dqkv = torch.zeros_like(qkv)
    fwd = t_ms(lambda: ops.attn_fwd(qkv, qkv[:, W:], qkv[:, 2 * W:], 3 * W, R, S, H, hd ** -0.5, out=out, **kw))
    bwd = t_ms(lambda: ops.attn_bwd(qkv, qkv[:, W:], qkv[:, 2 * W:], 3 * W, out, W, lse, do, W, dqkv, dqkv[:, W:], dqkv[:, 2 * W:], 3 * W, R, S, H, hd ** -0.5, **kw))
    os.environ["SVLA_ATTN96_F32"] = "0"
    return fwd, bwd, out.float(), dqkv.float()


# fusion layers of a 16 x 50 window (train mode), the decoder over a 50-step and a 256-step window
for name, R, S, causal, p in [("fusion  rows=800 S=181 dropout 0.1", 16 * 50, 181, False, 0.1), ("decoder rows=16  S=50  block-causal", 16, 50, True, 0.0),
                              ("decoder rows=16  S=256 block-causal", 16, 256, True, 0.0), ("fusion  rows=800 S=233 no dropout ", 16 * 50, 233, False, 0.0)]:
    f_new, b_new, o_new, g_new = one(R, S, 96, causal, p, False)
    f_old, b_old, o_old, g_old = one(R, S, 96, causal, p, True)
    f_64, b_64, _, _ = one(R, S, 64, causal, p, False)
    cos = torch.nn.functional.cosine_similarity(g_new.flatten(), g_old.flatten(), dim=0).item()
    print(f"{name}: forward  MFMA-96 {f_new:.3f} ms | fp32 detour {f_old:.3f} ms ({f_old / f_new:.1f}x) | 64-wide {f_64:.3f} ms (96 / 64 = {f_new / f_64:.2f})")
    print(f"{' ' * len(name)}  backward MFMA-96 {b_new:.3f} ms | fp32 detour {b_old:.3f} ms ({b_old / b_new:.1f}x) | 64-wide {b_64:.3f} ms (96 / 64 = {b_new / b_64:.2f})"
          f" | max |O diff| {(o_new - o_old).abs().max().item():.2e}, gradient cosine {cos:.6f}")
