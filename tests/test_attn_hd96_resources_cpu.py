"""Register / spill / scratch budget of the 96-wide attention kernels (csrc/attn_hd96.hip), checked at compile time with the flags of
tests/test_kernel_resources_cpu.py -- and the proof that the file cross-compiles for gfx950 on a machine without a GPU.

One workgroup is 4 waves, one per SIMD, so a kernel that is to run TWO workgroups per CU (the S <= 192 buckets: K + V = 72 KiB of LDS each) may use
at most 256 registers (arch VGPRs + AGPRs) per lane, and the S <= 256 bucket (96 KiB of LDS: one workgroup per CU) up to 512.  Dropout is a runtime
argument of the same kernels (``DropCfg::thr``), so "with and without dropout" is one code object per (bucket, masked?) pair: the zero-scratch
requirement of the no-dropout forward therefore holds for the dropout forward too."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers.kernel_resources import HIPCC, resources as _resources      # noqa: E402

# mangled-name fragment -> max registers per lane (VGPRs + AGPRs); the values of this build (in the comments) plus about 5 % slack, capped at what the
# bucket's occupancy allows.  VGPR spills and scratch are pinned at zero for every kernel of the file.
BUDGET = {
    "17attn96_fwd_kernelILi12ELb0E": 176,        # 165        fusion layers, S <= 192 (S = 181)
    "17attn96_fwd_kernelILi12ELb1E": 184,        # 175        masked form
    "17attn96_fwd_kernelILi16ELb0E": 304,        # 252 + 32   S <= 256 (one workgroup per CU)
    "17attn96_fwd_kernelILi16ELb1E": 312,        # 256 + 40
    "20attn96_bwd_dq_kernelILi12ELb0E": 176,     # 163
    "20attn96_bwd_dq_kernelILi12ELb1E": 176,     # 163
    "21attn96_bwd_dkv_kernelILi12ELb0E": 208,    # 191
    "21attn96_bwd_dkv_kernelILi12ELb1E": 208,    # 192
    "20attn96_bwd_dq_kernelILi16ELb0E": 296,     # 240 + 32
    "20attn96_bwd_dq_kernelILi16ELb1E": 296,     # 248 + 32
    "21attn96_bwd_dkv_kernelILi16ELb0E": 376,    # 256 + 96
    "21attn96_bwd_dkv_kernelILi16ELb1E": 376,    # 256 + 96
}
FIELDS = ("VGPRs", "AGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_attn_hd96_compiles_for_gfx950_within_its_register_budget():
    res = _resources("attn_hd96.hip")
    kernels = {k: v for k, v in res.items() if "attn96_" in k}
    assert len(kernels) == 24, sorted(kernels)                      # forward, dQ, dK/dV x four S buckets x (plain, masked)
    bad = []
    for k, v in kernels.items():
        assert all(f in v for f in FIELDS), (k, v)                  # every figure was parsed: a silent miss must not pass as zero
        regs = v["VGPRs"] + v["AGPRs"]
        two_per_cu = "ILi16E" not in k
        if v["VGPRs Spill"] or v["ScratchSize [bytes/lane]"] or regs > (256 if two_per_cu else 512):
            bad.append((k, v))
    for frag, max_regs in BUDGET.items():
        hits = {k: v for k, v in kernels.items() if frag in k}
        assert len(hits) == 1, (frag, sorted(kernels))
        for k, v in hits.items():
            print(f"{k}: {v}")
            if v["VGPRs"] + v["AGPRs"] > max_regs:
                bad.append((k, v, max_regs))
    assert not bad, bad
