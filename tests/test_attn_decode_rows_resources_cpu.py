"""Register / spill budget of the per-row KV-ring kernels (csrc/attn_decode_rows.hip), checked at compile time (hipcc cross-compiles gfx950 without a GPU; the
mechanism of tests/test_kernel_resources_cpu.py, the pattern of tests/test_decode_long_resources_cpu.py).

Both kernels and their grouped twins must not spill; the attention kernel holds eight 16-byte loads per thread in flight and must still fit 128 VGPRs (four waves
per SIMD at least: two workgroups of a (row, head) pair per CU and more)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers.kernel_resources import HIPCC, resources as _resources      # noqa: E402


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_rows_kernels_and_their_grouped_twins_do_not_spill():
    res = _resources("attn_decode_rows.hip")
    for kernel, max_vgprs in (("attn_decode_rows_kernel", 128), ("kv_append_rows_kernel", None)):
        single = {k: v for k, v in res.items() if kernel in k and "svla_grouped" not in k}
        twin = {k: v for k, v in res.items() if kernel + "_body" in k and "svla_grouped" in k}
        assert len(single) == 1 and len(twin) == 1, sorted(res)
        for k, v in {**single, **twin}.items():
            print(k[:80], v)
            assert v["VGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
            if max_vgprs is not None:
                assert v["VGPRs"] <= max_vgprs, (k, v)
