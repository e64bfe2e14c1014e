"""Register / spill / scratch / LDS budget of the long-sequence attention backward (csrc/attn_long.hip: head_dim 64, 256 < S <= 512), checked at compile time
with the flags of the build -- and the proof that the file cross-compiles for gfx950 on a machine without a GPU.

A workgroup is 8 waves (two per SIMD) and, with 64 .. 134.5 KiB of LDS, the only one on its CU: a wave may use up to 256 registers (arch VGPRs + AGPRs).
The LDS is dynamic (the remark reports 0 static bytes), so its size is restated here from the kernels' layout and held against the 160 KiB a single
workgroup may claim on gfx950."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers.kernel_resources import CSRC, HIPCC, resources as _resources      # noqa: E402

# mangled-name fragment -> (registers per lane measured with this build, pinned ceiling = measured + about 5 %)
BUDGET = {
    "23attn_long_bwd_dq_kernelILb0E": (116, 122),       # no mask
    "23attn_long_bwd_dq_kernelILb1E": (120, 126),       # block-causal / key padding
    "24attn_long_bwd_dkv_kernelILb0E": (156, 164),
    "24attn_long_bwd_dkv_kernelILb1E": (158, 166),
}
FIELDS = ("VGPRs", "AGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]")
LDS_PER_WORKGROUP = 160 * 1024


def _dynamic_lds(SP):
    """bytes the launcher asks for at padded length SP (al_lds_dq / al_lds_dkv): two [SP, 64] bf16 operands, trajectory ids, key mask (+ LSE and D)"""
    dq = 2 * SP * 64 * 2 + SP * (4 + 1)
    return dq, dq + SP * 2 * 4


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_attn_long_bwd_compiles_for_gfx950_without_spills_within_its_register_and_lds_budget():
    res = _resources("attn_long.hip")
    kernels = {k: v for k, v in res.items() if "attn_long_bwd_" in k}
    assert len(kernels) == 4, sorted(kernels)                       # dQ, dK/dV x (plain, masked)
    for frag, (measured, ceiling) in BUDGET.items():
        hits = {k: v for k, v in kernels.items() if frag in k}
        assert len(hits) == 1, (frag, sorted(kernels))
        (k, v), = hits.items()
        print(f"{k}: {v}")
        assert all(f in v for f in FIELDS), (k, v)                  # every figure was parsed: a silent miss must not pass as zero
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
        regs = v["VGPRs"] + v["AGPRs"]
        assert regs <= ceiling <= 256, (k, regs, measured, ceiling)  # 8 waves per workgroup = 2 per SIMD: 256 registers each
        dq, dkv = _dynamic_lds(512)
        assert v["LDS Size [bytes/block]"] + (dkv if "dkv" in k else dq) <= LDS_PER_WORKGROUP, (k, v)
    assert _dynamic_lds(512) == (133632, 137728)
    # the launcher's own arithmetic is the one restated above
    src = open(os.path.join(CSRC, "attn_long.hip")).read()
    assert "(size_t)2 * SP * AL_ROW * sizeof(bf16_t) + (size_t)SP * (sizeof(int) + 1)" in src and "al_lds_dq(SP) + (size_t)SP * 2 * sizeof(float)" in src
