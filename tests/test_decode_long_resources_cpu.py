"""Register / spill budget of the single-query attention kernels, checked at compile time (hipcc cross-compiles gfx950 without a GPU; the mechanism of
tests/test_kernel_resources_cpu.py).

The long-window kernel (csrc/attn_decode_long.hip, 512 < S <= 1024) keeps its scores in LDS because 32 per-block scores in registers next to the loads in flight
would not fit: it and its grouped twin must not spill.  The existing kernel for S <= 512 (csrc/attn.hip: attn_decode_kernel) carries the 64-env policy step and
must compile as it did before the long window was added: 50 VGPRs, no scratch, single-launch kernel and grouped twin alike."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers.kernel_resources import HIPCC, resources as _resources      # noqa: E402

DECODE_VGPRS = 50           # attn_decode_kernel and its grouped twin before this kernel existed


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_long_decode_kernel_and_its_grouped_twin_do_not_spill():
    res = _resources("attn_decode_long.hip")
    single = {k: v for k, v in res.items() if "attn_decode_long_kernel" in k and "svla_grouped" not in k}
    twin = {k: v for k, v in res.items() if "attn_decode_long_kernel_body" in k and "svla_grouped" in k}
    assert len(single) == 1 and len(twin) == 1, sorted(res)
    for k, v in {**single, **twin}.items():
        print(k[:80], v)
        assert v["VGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
        assert v["VGPRs"] <= 128, (k, v)            # four waves per SIMD at least: two workgroups of a (row, head) pair per CU and more


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_existing_decode_kernel_compiles_as_before():
    res = _resources("attn.hip")
    hits = {k: v for k, v in res.items() if "attn_decode_kernel" in k}
    assert len(hits) == 2, sorted(hits)             # attn_decode_kernel(AttnArgs) and svla_grouped<&attn_decode_kernel_body, ...>
    for k, v in hits.items():
        print(k[:80], v)
        assert v["VGPRs"] <= DECODE_VGPRS and v["VGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
