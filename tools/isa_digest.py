#!/usr/bin/env python3
"""sha256 of the gfx950 device assembly of every csrc/*.hip, compiled with the flags of the build (safevla_amd/build.py: BASE_FLAGS): equal digests before and
after a change mean the compiler emitted the same device code, so the change cannot move results or speed.  Needs hipcc and a built tree (gemm.hip includes the
generated _obj/gelu_poly.h), no GPU.
  python tools/isa_digest.py [--kernels] [--root OTHER_CHECKOUT]      --kernels: one more line per kernel; --root: digest another checkout with THIS tree's flags
Only the lines that name the per-compilation symbol __hip_cuid_<hash> are dropped before hashing; the text is hashed, not inspected."""
import argparse
import glob
import hashlib
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from safevla_amd.build import BASE_FLAGS, HIPCC      # noqa: E402


def device_asm(root, src):
    csrc = os.path.join(root, "safevla_amd", "csrc")
    r = subprocess.run([HIPCC, *BASE_FLAGS, "--cuda-device-only", "-S", "-I", os.path.join(root, "include"), src, "-o", "-"], capture_output=True, text=True, cwd=csrc)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}:\n{r.stderr[-3000:]}")
    return "".join(l for l in r.stdout.splitlines(keepends=True) if "__hip_cuid_" not in l)


def sha(text):
    return hashlib.sha256(text.encode()).hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--kernels", action="store_true", help="also print one digest per function (label .. .Lfunc_end)")
    ap.add_argument("--root", default=HERE, help="checkout whose csrc/ is compiled (default: this one)")
    a = ap.parse_args()
    srcs = sorted(os.path.basename(s) for s in glob.glob(os.path.join(a.root, "safevla_amd", "csrc", "*.hip")))
    with ThreadPoolExecutor(max_workers=8) as ex:
        asms = list(ex.map(lambda s: device_asm(a.root, s), srcs))
    for src, asm in zip(srcs, asms):
        print(f"{sha(asm)}  {src}")
        if a.kernels:
            for m in re.finditer(r"^(\w+):.*?^\.Lfunc_end\d+:", asm, flags=re.M | re.S):
                print(f"    {sha(m.group(0))}  {m.group(1)}")


if __name__ == "__main__":
    main()
