"""Register / scratch figures of the antialiased bicubic resize kernel (csrc/resize.hip), read from the compiled gfx950 code object (hipcc cross-compiles without a
GPU; the mechanism of tests/test_conv_resources_cpu.py).

The kernel keeps its tap weights in LDS, not in a per-thread array (the tap count is a run-time value: an array indexed by it would live in scratch), so it may use
no scratch and spill nothing.  Its LDS is dynamic -- sized per geometry by the host, at most 48 KiB -- so the static figure is 0.  It is a memory-bound stream:
at most 72 VGPRs keeps seven waves per SIMD."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers.kernel_resources import HIPCC, resources as _resources      # noqa: E402

VGPRS = 68      # found when this was written


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_resize_kernel_registers_and_scratch():
    res = _resources("resize.hip")
    assert len(res) == 1, sorted(res)
    (name, v), = res.items()
    print(name, v)
    assert "resize_bicubic_aa_u8_kernel" in name
    assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, v
    assert v["VGPRs"] == VGPRS <= 72, v
    assert v["LDS Size [bytes/block]"] == 0, v
