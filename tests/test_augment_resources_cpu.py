"""Register / scratch / LDS figures of the frame-augmentation kernels (csrc/augment.hip), read from the compiled gfx950 code object (hipcc cross-compiles without a
GPU; the mechanism of tests/test_attn_decode_resources_cpu.py).

The three kernels index no array dynamically (operation codes, factors and blur weights are scalar kernel arguments selected by unrolled code), so none may use
scratch; their LDS is static: the staged chunk of the gray reduction, the jitter tile with its blur halo, the crop source rectangle plus the resized tile with its
sharpness halo.  All three must keep at least four waves per SIMD (128 VGPRs): they are memory-bound streams that live on occupancy."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers.kernel_resources import HIPCC, resources as _resources      # noqa: E402

# kernel -> (VGPRs at most, LDS bytes per block exactly)
PINS = {
    "aug_gray_partials_kernel": (40, 2048 * 3 + 16 + 4 * 8),                                              # 38 VGPRs when this was written
    "aug_jitter_blur_kernel": (88, 24 * ((128 + 4) * 3 + 12) + 24 + 4),                                   # 80
    "aug_resize_post_sharp_kernel": (32, 20 * ((128 + 4) * 3 + 12) + 18 * ((128 + 2) * 3 + 2) + 20),      # 25
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_augment_kernels_registers_scratch_and_lds():
    res = _resources("augment.hip")
    assert len(res) == 3, sorted(res)
    for name, (vgprs, lds) in PINS.items():
        hits = [v for k, v in res.items() if name in k]
        assert len(hits) == 1, (name, sorted(res))
        v = hits[0]
        print(name, v)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)
        assert v["VGPRs"] <= vgprs <= 128, (name, v)
        assert v["LDS Size [bytes/block]"] == lds, (name, v, lds)
