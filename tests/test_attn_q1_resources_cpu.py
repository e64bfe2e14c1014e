"""Register / spill / scratch / LDS budget of the two streaming kernels of the absorbed last fusion layer (csrc/attn_q1.hip), checked at compile time with the
flags of the build -- and the proof that the file cross-compiles for gfx950 on a machine without a GPU.

A workgroup is 8 waves (two per SIMD) and holds its row's tokens in registers (32 slots x 4 registers per lane) next to 64 accumulators: it is the only workgroup
on its CU by registers, so a wave may use up to 256 (arch VGPRs + AGPRs).  The LDS is dynamic (the remark reports 0 static bytes): its size is restated here from
the kernels' layout and held against the 160 KiB a single workgroup may claim on gfx950."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers.kernel_resources import CSRC, HIPCC, resources as _resources      # noqa: E402

# mangled-name fragment -> (registers per lane measured with this build, pinned ceiling = measured + about 5 %)
BUDGET = {
    "18attn_q1_fwd_kernel": (204, 214),
    "18attn_q1_bwd_kernel": (206, 216),
}
FIELDS = ("VGPRs", "AGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]")
LDS_PER_WORKGROUP = 160 * 1024
SMAX, H, D = 256, 8, 512
# [SMAX][8] fp32 coefficient tables (forward: one, backward: two) + four [8, 512] fp32 buffers of the cross-wave sum
DYNAMIC_LDS = {"fwd": (SMAX * H + 4 * H * D) * 4, "bwd": (2 * SMAX * H + 4 * H * D) * 4}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_attn_q1_compiles_for_gfx950_without_spills_within_its_register_and_lds_budget():
    res = _resources("attn_q1.hip")
    kernels = {k: v for k, v in res.items() if "attn_q1_" in k}
    assert len(kernels) == 2, sorted(kernels)
    for frag, (measured, ceiling) in BUDGET.items():
        hits = {k: v for k, v in kernels.items() if frag in k}
        assert len(hits) == 1, (frag, sorted(kernels))
        (k, v), = hits.items()
        print(f"{k}: {v}")
        assert all(f in v for f in FIELDS), (k, v)                  # every figure was parsed: a silent miss must not pass as zero
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
        regs = v["VGPRs"] + v["AGPRs"]
        assert regs == measured, (k, regs, measured)                # the figure the build shows; a change of it is a change of the kernel
        assert regs <= ceiling <= 256, (k, regs, ceiling)           # 8 waves per workgroup = 2 per SIMD: 256 registers each
        assert v["LDS Size [bytes/block]"] + DYNAMIC_LDS["bwd" if "bwd" in k else "fwd"] <= LDS_PER_WORKGROUP, (k, v)
    assert DYNAMIC_LDS == {"fwd": 73728, "bwd": 81920}
    # the launcher's own arithmetic is the one restated above
    src = open(os.path.join(CSRC, "attn_q1.hip")).read()
    assert "#define Q1_LDS_FWD ((size_t)(Q1_SMAX * Q1_H + 4 * Q1_RED_FLOATS) * sizeof(float))" in src
    assert "#define Q1_LDS_BWD ((size_t)(2 * Q1_SMAX * Q1_H + 4 * Q1_RED_FLOATS) * sizeof(float))" in src
    # the small head_expand / head_pick kernels of the same file: no spills either
    for k, v in res.items():
        if "head_expand_kernel" in k or "head_pick_kernel" in k:
            assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
