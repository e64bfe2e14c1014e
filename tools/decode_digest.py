#!/usr/bin/env python3
"""Digests of what the three single-query attention kernels (csrc/attn_decode.hip) compute, for a fixed list of small cases.  The output-side sibling of
tools/isa_digest.py: equal lines before and after a change of those kernels mean that every case came out bit for bit the same.  Needs a GPU and a built tree;
one process, a second or two.
  python tools/decode_digest.py [--root OTHER_CHECKOUT]
--root: the same cases against another checkout's safevla_amd/ package and its own built library, in a child interpreter.

Cases: 5 rows, H in {2, 8}, S (the cache window) in {1, 33, 512, 513, 1024}, four key sets each.  Inputs are seeded on the CPU and exact in bf16.
  fwd    ops.attn_fwd(Sq = 1, kvalid): attn_decode_kernel for S <= 512, attn_decode_long_kernel above.  Key sets: none, the last key alone, the window
         [S / 4, S / 4 + S / 2), all (kvalid None)
  rows   ops.attn_decode_rows(klen, cache_row): attn_decode_rows_kernel.  Key sets: klen = 0, 1, S / 2 and S (and S + 5 on one row of ``all``: clamped), each
         with cache_row None and with a permutation into an 8-row cache
One line per case: sha256 over the bytes of O, then of LSE.  The tool hashes and prints; it inspects nothing."""
import argparse
import hashlib
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
ROWS, HD, CACHE = 5, 64, 8
PERM = [6, 2, 7, 0, 3]


def run(root):
    sys.path.insert(0, root)
    import torch

    from safevla_amd import ops

    print(f"# decode digest of {os.path.relpath(root, HERE)}")

    def rnd(seed, *shape):
        return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).bfloat16().to(DEV)

    def line(name, o, lse):
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for t in (o, lse):
            h.update(t.contiguous().cpu().view(torch.uint8).numpy().tobytes())
        print(f"{name:<44} {h.hexdigest()}", flush=True)

    for H in (2, 8):
        D = H * HD
        for S in (1, 33, 512, 513, 1024):
            kv, q = rnd(100 + S + H, CACHE * S, 2 * D), rnd(200 + S + H, ROWS, 3 * D)      # the query: the first third of a fused qkv row
            sets = {"none": torch.zeros(ROWS, S, dtype=torch.uint8), "last": torch.zeros(ROWS, S, dtype=torch.uint8), "mid": torch.zeros(ROWS, S, dtype=torch.uint8),
                    "all": None}
            sets["last"][:, S - 1] = 1
            sets["mid"][:, S // 4:S // 4 + max(S // 2, 1)] = 1
            for name, kvalid in sets.items():
                o, lse = ops.attn_fwd(q, kv, kv[:, D:], 2 * D, ROWS, S, H, 0.125, kvalid=None if kvalid is None else kvalid.to(DEV), save_lse=True, Sq=1,
                                      ldq=3 * D, kv_rows=S)
                line(f"fwd  H={H} S={S} keys={name}", o, lse)
            for name, n in (("none", 0), ("one", 1), ("mid", max(S // 2, 1)), ("all", S)):
                klen = torch.full((ROWS,), n, dtype=torch.int32)
                if name == "all":
                    klen[2] = S + 5
                for perm in (False, True):
                    crow = torch.tensor(PERM, dtype=torch.int32, device=DEV) if perm else None
                    o, lse = ops.attn_decode_rows(q, 3 * D, kv, kv[:, D:], 2 * D, klen.to(DEV), crow, ROWS, H, 0.125, S, save_lse=True)
                    line(f"rows H={H} S={S} keys={name} perm={int(perm)}", o, lse)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--root", default=HERE, help="checkout whose safevla_amd/ package and library run the cases (default: this one)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    if root != HERE and not a.child:      # another checkout's package: a fresh interpreter that never imported this tree's
        sys.exit(subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--child"]).returncode)
    run(root)


if __name__ == "__main__":
    main()
