"""Registers, LDS and spills of the single-query attention family (csrc/attn_decode.hip), checked at compile time (hipcc cross-compiles gfx950 without a GPU; the
mechanism of tests/test_kernel_resources_cpu.py).

The three attention kernels share their arithmetic as inlined helpers and differ in how they walk the keys; what the helpers cost shows here.  Each kernel and its
grouped twin must compile to the figures recorded when the three were separate copies (profiles/attn_decode_isa.txt): no more VGPRs, the same LDS, no scratch, no
spill.  attn_decode_kernel carries the 64-env policy step; the two LDS-score kernels hold eight 16-byte loads per thread in flight next to their accumulators, and
the long one went from 73 to 102 VGPRs (six waves per SIMD to four) when its P.V step was first taken through a helper.  kv_append_rows_kernel must not spill."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers.kernel_resources import HIPCC, resources as _resources      # noqa: E402

#          kernel                    (VGPRs <=, LDS bytes ==)
RECORDED = {"attn_decode_kernel": (50, 1056),
            "attn_decode_long_kernel": (73, 6192),
            "attn_decode_rows_kernel": (71, 5152),
            "kv_append_rows_kernel": (None, 0)}


@pytest.fixture(scope="module")
def res():
    return _resources("attn_decode.hip")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
@pytest.mark.parametrize("kernel", list(RECORDED))
def test_kernel_and_its_grouped_twin_compile_as_recorded(res, kernel):
    # exact names: the mangled form carries the length, so "attn_decode_kernel" cannot pick up attn_decode_long_kernel or a _body
    single = {k: v for k, v in res.items() if k.startswith(f"_Z{len(kernel)}{kernel}") and "svla_grouped" not in k}
    twin = {k: v for k, v in res.items() if f"_Z{len(kernel) + 5}{kernel}_body" in k and "svla_grouped" in k}
    assert len(single) == 1 and len(twin) == 1, sorted(res)
    max_vgprs, lds = RECORDED[kernel]
    for k, v in {**single, **twin}.items():
        print(k[:80], v)
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
        assert v["LDS Size [bytes/block]"] == lds, (k, v)
        if max_vgprs is not None:
            assert v["VGPRs"] <= max_vgprs, (k, v)
