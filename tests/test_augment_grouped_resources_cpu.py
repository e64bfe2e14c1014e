"""Register / scratch / LDS figures of the grouped frame-augmentation kernels (csrc/augment_grouped.hip), read from the compiled gfx950 code object (the
mechanism of tests/helpers/kernel_resources.py; hipcc cross-compiles without a GPU).

The grouped kernels are the three kernels of csrc/augment.hip with their parameters read from a table entry instead of the kernel arguments.  A block serves one
image, so the entry's address is uniform and the parameters must arrive as the kernel arguments do: in scalar registers.  Parameters that ended up in vector
registers or scratch would show here as a higher VGPR count or a scratch size; the table is not staged in LDS, so the LDS sizes are exactly those of augment.hip."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers.kernel_resources import HIPCC, resources as _resources      # noqa: E402

# kernel -> (VGPRs exactly as measured when this was written, LDS bytes per block exactly: the figures of tests/test_augment_resources_cpu.py)
PINS = {
    "aug_gray_partials_grouped_kernel": (38, 2048 * 3 + 16 + 4 * 8),                                              # 6 192 B; augment.hip's kernel: 38 VGPRs
    "aug_jitter_blur_grouped_kernel": (79, 24 * ((128 + 4) * 3 + 12) + 24 + 4),                                   # 9 820 B; 80 (the grouped form has no blur-off path)
    "aug_resize_post_sharp_grouped_kernel": (25, 20 * ((128 + 4) * 3 + 12) + 18 * ((128 + 2) * 3 + 2) + 20),      # 15 236 B; 25
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_grouped_augment_kernels_registers_scratch_and_lds():
    res = _resources("augment_grouped.hip")
    assert len(res) == 3, sorted(res)
    for name, (vgprs, lds) in PINS.items():
        hits = [v for k, v in res.items() if name in k]
        assert len(hits) == 1, (name, sorted(res))
        v = hits[0]
        print(name, v)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)
        assert v["VGPRs"] == vgprs, (name, v)
        assert v["LDS Size [bytes/block]"] == lds, (name, v, lds)
