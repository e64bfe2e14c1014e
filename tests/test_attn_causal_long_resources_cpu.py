"""Register / spill / LDS budget of the streaming causal attention forward (csrc/attn_seq_long.hip), checked at compile time (hipcc cross-compiles gfx950 without a
GPU; the mechanism of tests/test_kernel_resources_cpu.py, the pattern of tests/test_attn_decode_resources_cpu.py).

The kernel and its grouped twin must not spill or use scratch; their LDS (all of it static: two K + V tile buffers and the trajectory ids, no dynamic part) must let
two workgroups share a CU's 160 KiB; and they stay at or below the 117 VGPRs both compiled to on 2026-10-20 (four workgroups of four waves per CU)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers.kernel_resources import HIPCC, resources as _resources      # noqa: E402

CU_LDS = 160 * 1024
MAX_VGPRS = 117      # 2026-10-20


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_causal_long_kernel_and_its_grouped_twin():
    res = _resources("attn_seq_long.hip")
    single = {k: v for k, v in res.items() if "attn_causal_long_kernel" in k and "svla_grouped" not in k}
    twin = {k: v for k, v in res.items() if "attn_causal_long_kernel_body" in k and "svla_grouped" in k}
    assert len(single) == 1 and len(twin) == 1, sorted(res)
    for k, v in {**single, **twin}.items():
        print(k[:80], v)
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
        assert 2 * v["LDS Size [bytes/block]"] <= CU_LDS, (k, v)      # the launch passes 0 bytes of dynamic LDS
        assert v["VGPRs"] <= MAX_VGPRS, (k, v)
