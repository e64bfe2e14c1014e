"""What the compiler did with the kernels of one csrc/*.hip file, read from -Rpass-analysis=kernel-resource-usage (hipcc cross-compiles gfx950 without a GPU).

The one parser behind the tests/test_*_resources_cpu.py files.  The device side is compiled with the flag list of the build itself (safevla_amd/build.py:
BASE_FLAGS), so the figures are those of the code that ships.  ``resources(src)`` returns {mangled kernel name: {field: int}} with every integer field the remark
prints: SGPRs, VGPRs, AGPRs, ScratchSize [bytes/lane], Occupancy [waves/SIMD], SGPRs Spill, VGPRs Spill, LDS Size [bytes/block]."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from safevla_amd.build import BASE_FLAGS, CSRC, HIPCC      # noqa: E402  (build.py imports no torch)

FLAGS = BASE_FLAGS + ["--cuda-device-only", "-c"]


def resources(src):
    r = subprocess.run([HIPCC, *FLAGS, "-I", os.path.join(ROOT, "include"), os.path.join(CSRC, src), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stderr[-3000:]
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(?:\S+:\d+:\d+:\s+)?([A-Za-z][^:]*): (\d+)\b", line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    return out
