"""Register / spill budget of the hot HIP kernels, checked at compile time (hipcc cross-compiles gfx950 without a GPU).

Round 6 found a 5.6 % regression of the whole update by an A/B against the previous round's tree: wrapping the attention forward kernels' bodies in same-named
__global__ functions (for the tower-grouped launches) made `attn_fwd_persist_kernel<12>` spill 109 VGPRs instead of 6 and run 2x slower, while every parity test stayed
green.  This test pins what the compiler does with the kernels that carry the update: VGPR count (= occupancy) and spill counts from -Rpass-analysis=kernel-resource-usage."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers.kernel_resources import HIPCC, resources as _resources      # noqa: E402

# kernel-name fragment (mangled) -> (max VGPRs, max spilled VGPRs): the values of the round-6 build with a little slack; a change of schedule that needs more is a
# decision to take with an A/B in hand (tools/ab_attn.py, bench.py against the previous tree), not something to discover in a profile a round later
BUDGET = {
    "attn.hip": {
        "28attn_fwd_persist_kernel_bodyILi12E": (256, 12),             # the fusion attention forward of the update (2 workgroups per CU)
        "27attn_bwd_fused_exact_kernelILi12ELb1E": (170, 8),           # its backward with dropout: THREE workgroups per CU need <= 170
        "27attn_bwd_fused_exact_kernelILi12ELb0E": (170, 8),
        "20attn_fwd_kernel_bodyILi18ELb0ELi4ELb1E": (176, 0),          # the ViT at 224 x 224 (S = 257): two workgroups per CU
        "20attn_fwd_kernel_bodyILi28ELb0ELi8ELb1E": (216, 0),          # the ViT's S = 433 attention
    },
    "gemm.hip": {
        "19gemm_nt_bf16_kernel10GemmNtArgs": (192, 0),                 # 128-tile kernel (two workgroups per CU)
        "21gemm_nt8p_bf16_kernelILi0ELi1ELb1EE": (256, 0),             # linear2 / out_proj forward with residual + dropout
        "21gemm_nt8p_bf16_kernelILi1ELi0ELb1EE": (256, 0),
        "26gemm_nt8p_bf16_kernel_bodyILi0ELi0ELb0EE": (256, 0),        # grouped twins must match their single-launch kernels
        "24gemm_nt_bf16_kernel_body10GemmNtArgs": (192, 0),
    },
    "norm.hip": {
        "15norm_fwd_kernelItLi512EE": (64, 0),
        "15norm_bwd_kernelItLi512EE": (128, 4),
    },
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_hot_kernels_keep_their_register_budget():
    with ThreadPoolExecutor(max_workers=len(BUDGET)) as ex:
        res = dict(zip(BUDGET, ex.map(_resources, BUDGET)))
    bad = []
    for src, kernels in BUDGET.items():
        for frag, (max_vgpr, max_spill) in kernels.items():
            hits = {k: v for k, v in res[src].items() if frag in k}
            assert hits, (src, frag, sorted(res[src])[:5])
            for k, v in hits.items():
                if v.get("VGPRs", 0) > max_vgpr or v.get("VGPRs Spill", 0) > max_spill:
                    bad.append((k[:90], v, (max_vgpr, max_spill)))
    assert not bad, bad
