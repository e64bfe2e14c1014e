"""Register / scratch / LDS figures of the validation-metrics kernel (csrc/metrics.hip), read from the compiled gfx950 code object (hipcc cross-compiles without a
GPU; the one parser of tests/helpers/kernel_resources.py).

The kernel is a handful of wave reductions per row: no scratch, nothing spilled.  Its LDS is static and is what DESIGN.md section 4n states: the 64 x 64 int
histogram (16 384 bytes, of which a launch uses the first A x A cells) plus one fp64 partial per wave and sum (4 x 3 x 8 = 96 bytes) = 16 480 bytes per workgroup."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers.kernel_resources import HIPCC, resources as _resources      # noqa: E402

LDS = 64 * 64 * 4 + 4 * 3 * 8


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_action_metrics_kernel_registers_scratch_and_lds():
    res = _resources("metrics.hip")
    assert len(res) == 1, sorted(res)
    (name, v), = res.items()
    print(name, v)
    assert "action_metrics_kernel" in name
    assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, v
    assert v["LDS Size [bytes/block]"] == LDS == 16480, v
    assert v["VGPRs"] <= 64, v                         # eight waves per SIMD (found when this was written: 38)
    design = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "DESIGN.md")).read()
    assert "16 480 bytes" in design[design.index("## 4n"):]
