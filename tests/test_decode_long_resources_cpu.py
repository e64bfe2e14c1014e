"""Register / spill budget of the single-query attention kernels, checked at compile time (hipcc cross-compiles gfx950 without a GPU; the mechanism of
tests/test_kernel_resources_cpu.py).

The long-window kernel (csrc/attn_decode_long.hip, 512 < S <= 1024) keeps its scores in LDS because 32 per-block scores in registers next to the loads in flight
would not fit: it and its grouped twin must not spill.  The existing kernel for S <= 512 (csrc/attn.hip: attn_decode_kernel) carries the 64-env policy step and
must compile as it did before the long window was added: 50 VGPRs, no scratch, single-launch kernel and grouped twin alike."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "safevla_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-mllvm", "-amdgpu-mfma-vgpr-form=1", "--cuda-device-only", "-c"]
DECODE_VGPRS = 50           # attn_decode_kernel and its grouped twin before this kernel existed


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
        m = re.search(r"remark:\s+(?:\S+\s+)?(VGPRs|VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_long_decode_kernel_and_its_grouped_twin_do_not_spill():
    res = _resources("attn_decode_long.hip")
    single = {k: v for k, v in res.items() if "attn_decode_long_kernel" in k and "svla_grouped" not in k}
    twin = {k: v for k, v in res.items() if "attn_decode_long_kernel_body" in k and "svla_grouped" in k}
    assert len(single) == 1 and len(twin) == 1, sorted(res)
    for k, v in {**single, **twin}.items():
        print(k[:80], v)
        assert v["VGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
        assert v["VGPRs"] <= 128, (k, v)            # four waves per SIMD at least: two workgroups of a (row, head) pair per CU and more


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_existing_decode_kernel_compiles_as_before():
    res = _resources("attn.hip")
    hits = {k: v for k, v in res.items() if "attn_decode_kernel" in k}
    assert len(hits) == 2, sorted(hits)             # attn_decode_kernel(AttnArgs) and svla_grouped<&attn_decode_kernel_body, ...>
    for k, v in hits.items():
        print(k[:80], v)
        assert v["VGPRs"] <= DECODE_VGPRS and v["VGPRs Spill"] == 0 and v["ScratchSize [bytes/lane]"] == 0, (k, v)
