"""Register / scratch / LDS figures of the convolution kernels of the frozen CLIP RN50 trunk (csrc/conv.hip), read from the compiled gfx950 code object (hipcc
cross-compiles without a GPU; the mechanism of tests/test_augment_resources_cpu.py).

No kernel of the file may use scratch or spill (the stem once did both: its 864 lane-uniform weights were hoisted into scalar registers, 806 of them spilled; with the
tap loop unrolled the LDS copy of them was prefetched into 352 spilled VGPRs).  The implicit-GEMM kernel's registers and static LDS -- two buffers of (128 pixel + BN
weight) rows of 64 bytes -- are pinned per channel-tile width: two blocks per CU need <= 128 VGPRs at four waves per block and SIMD."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "safevla_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-mllvm", "-amdgpu-mfma-vgpr-form=1", "--cuda-device-only", "-c"]
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


def _resources(src):
    r = subprocess.run([HIPCC, *FLAGS, "-I", os.path.join(ROOT, "include"), os.path.join(CSRC, src), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stderr[-3000:]
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(?:\S+\s+)?(VGPRs|VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    return out


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
