"""Register / scratch figures of the antialiased bicubic resize kernel (csrc/resize.hip), read from the compiled gfx950 code object (hipcc cross-compiles without a
GPU; the mechanism of tests/test_conv_resources_cpu.py).

The kernel keeps its tap weights in LDS, not in a per-thread array (the tap count is a run-time value: an array indexed by it would live in scratch), so it may use
no scratch and spill nothing.  Its LDS is dynamic -- sized per geometry by the host, at most 48 KiB -- so the static figure is 0.  It is a memory-bound stream:
at most 72 VGPRs keeps seven waves per SIMD."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "safevla_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-mllvm", "-amdgpu-mfma-vgpr-form=1", "--cuda-device-only", "-c"]
VGPRS = 68      # found when this was written


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
def test_resize_kernel_registers_and_scratch():
    res = _resources("resize.hip")
    assert len(res) == 1, sorted(res)
    (name, v), = res.items()
    print(name, v)
    assert "resize_bicubic_aa_u8_kernel" in name
    assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, v
    assert v["VGPRs"] == VGPRS <= 72, v
    assert v["LDS Size [bytes/block]"] == 0, v
