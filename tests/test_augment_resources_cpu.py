"""Register / scratch / LDS figures of the six frame-augmentation kernels (csrc/augment.hip), read from the compiled gfx950 code object (hipcc cross-compiles
without a GPU; the mechanism of tests/helpers/kernel_resources.py).  The file is compiled once for both launch forms.

Single-transform kernels.  They index no array dynamically (operation codes, factors and blur weights are scalar kernel arguments selected by unrolled code), so
none may use scratch; their LDS is static: the staged chunk of the gray reduction, the jitter tile with its blur halo, the crop source rectangle plus the resized
tile with its sharpness halo.  All three must keep at least four waves per SIMD (128 VGPRs): they are memory-bound streams that live on occupancy.

Grouped kernels.  They call the same three device bodies with their parameters read from a table entry instead of the kernel arguments.  A block serves one image,
so the entry's address is uniform and the parameters must arrive as the kernel arguments do: in scalar registers.  Parameters that ended up in vector registers or
scratch would show here as a higher VGPR count or a scratch size; the table is not staged in LDS, so the LDS sizes are exactly those of the single-transform kernels."""
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

# kernel -> (VGPRs exactly as measured when this was written, LDS bytes per block exactly: the figures of PINS)
GROUPED_PINS = {
    "aug_gray_partials_grouped_kernel": (38, 2048 * 3 + 16 + 4 * 8),                                              # 6 192 B; the single-transform kernel: 38 VGPRs
    "aug_jitter_blur_grouped_kernel": (79, 24 * ((128 + 4) * 3 + 12) + 24 + 4),                                   # 9 820 B; 80 (the grouped form has no blur-off path)
    "aug_resize_post_sharp_grouped_kernel": (25, 20 * ((128 + 4) * 3 + 12) + 18 * ((128 + 2) * 3 + 2) + 20),      # 15 236 B; 25
}


@pytest.fixture(scope="module")
def res():
    if not os.path.exists(HIPCC):
        pytest.skip("needs hipcc")
    res = _resources("augment.hip")
    assert len(res) == 6, sorted(res)
    return res


def _kernel(res, name):
    hits = [v for k, v in res.items() if name in k]
    assert len(hits) == 1, (name, sorted(res))
    v = hits[0]
    print(name, v)
    assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)
    return v


def test_augment_kernels_registers_scratch_and_lds(res):
    for name, (vgprs, lds) in PINS.items():
        v = _kernel(res, name)
        assert v["VGPRs"] <= vgprs <= 128, (name, v)
        assert v["LDS Size [bytes/block]"] == lds, (name, v, lds)


def test_grouped_augment_kernels_registers_scratch_and_lds(res):
    for name, (vgprs, lds) in GROUPED_PINS.items():
        v = _kernel(res, name)
        assert v["VGPRs"] == vgprs, (name, v)
        assert v["LDS Size [bytes/block]"] == lds, (name, v, lds)
