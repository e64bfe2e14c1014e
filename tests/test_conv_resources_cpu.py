"""Register / scratch / LDS figures of the convolution kernels of the frozen CLIP RN50 trunk (csrc/conv.hip), read from the compiled gfx950 code object (hipcc
cross-compiles without a GPU; the mechanism of tests/test_augment_resources_cpu.py).

No kernel of the file may use scratch or spill (the stem once did both: its 864 lane-uniform weights were hoisted into scalar registers, 806 of them spilled; with the
tap loop unrolled the LDS copy of them was prefetched into 352 spilled VGPRs).  The implicit-GEMM kernel's registers and static LDS -- two buffers of (128 pixel + BN
weight) rows of 64 bytes -- are pinned per channel-tile width: two blocks per CU need <= 128 VGPRs at four waves per block and SIMD."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers.kernel_resources import HIPCC, resources as _resources      # noqa: E402

# kernel -> (VGPRs exactly, LDS bytes per block exactly)
PINS = {
    "conv_igemm_bf16_kernelILi128E": (127, 2 * (128 + 128) * 64),      # 127 VGPRs when this was written
    "conv_igemm_bf16_kernelILi64E": (88, 2 * (128 + 64) * 64),         # 88
    "conv_igemm_bf16_kernelILi32E": (60, 2 * (128 + 32) * 64),         # 60
}
# kernel -> (VGPRs at most, LDS bytes per block exactly)
STREAMS = {
    "conv_stem_u8_bf16_kernel": (128, 27 * 32 * 4),                    # 108 VGPRs when this was written
    "avgpool2_nhwc_bf16_kernel": (64, 0),                              # 30
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_conv_kernels_registers_scratch_and_lds():
    res = _resources("conv.hip")
    assert len(res) == 5, sorted(res)
    for name, v in res.items():
        print(name, v)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)
    for name, (vgprs, lds) in PINS.items():
        hits = [v for k, v in res.items() if name in k]
        assert len(hits) == 1, (name, sorted(res))
        assert hits[0]["VGPRs"] == vgprs <= 128, (name, hits[0])
        assert hits[0]["LDS Size [bytes/block]"] == lds, (name, hits[0], lds)
    for name, (vgprs, lds) in STREAMS.items():
        hits = [v for k, v in res.items() if name in k]
        assert len(hits) == 1, (name, sorted(res))
        assert hits[0]["VGPRs"] <= vgprs, (name, hits[0])
        assert hits[0]["LDS Size [bytes/block]"] == lds, (name, hits[0], lds)
