"""Per-launch times of the last fusion layer's attention at update size, absorbed (csrc/attn_q1.hip + the head-expanded GEMMs) against materialised (K / V GEMM,
single-query attention, dK/dV weight-gradient GEMM, dX GEMM), on one device in one process.  Device events around each launch, median of --iters after a warm-up.

    python tools/ab_attn_q1.py [--rows 16384] [--S 181] [--p 0.1] [--iters 7] [--only fwd|bwd|both]

``--only`` issues just the two streaming kernels in a loop (for a counter pass of the profiler: FETCH_SIZE / WRITE_SIZE in runs of their own)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from safevla_amd import ops      # noqa: E402

D, H = 512, 8


def timed(fn, iters):
    for _ in range(2):
        fn()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--S", type=int, default=181)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--only", choices=["fwd", "bwd", "both"], default=None)
    a = ap.parse_args()
    R, S, M, dev, bf = a.rows, a.S, a.rows * a.S, "cuda", torch.bfloat16
    scale = 64 ** -0.5
    torch.manual_seed(0)
    x = torch.randn(R, S, D, device=dev, dtype=bf)
    q0 = torch.randn(R, D, device=dev, dtype=bf)
    dao = torch.randn(R, D, device=dev, dtype=bf)
    W = (torch.randn(3 * D, D, device=dev) * D ** -0.5).to(bf)
    Wt = W.t().contiguous()
    b = torch.randn(3 * D, device=dev) * 0.5
    dW, db = torch.zeros(3 * D, D, device=dev), torch.zeros(3 * D, device=dev)
    drop = ops.Dropout(1234, 8, a.p) if a.p > 0 else None
    xf = x.view(M, D)

    # absorbed: every intermediate once, then each launch on its own
    eq, _, _ = ops.head_expand(q0, R)
    qt = ops.gemm_nt(eq, Wt[:, D:2 * D], 8 * R, D, D)
    c, sig, P = ops.attn_q1_fwd(x, S * D, qt, R, S, scale, drop=drop)
    go = ops.gemm_nt(c, W[2 * D:], 8 * R, D, D)
    edao, dsig, sdao = ops.head_expand(dao, R, bias=b[2 * D:], sigma=sig)
    dc = ops.gemm_nt(edao, Wt[:, 2 * D:], 8 * R, D, D)
    dx, dqt = ops.attn_q1_bwd(x, S * D, qt, dc, dsig, P, R, S, scale, drop=drop)
    gq = ops.gemm_nt(dqt, W[D:2 * D], 8 * R, D, D)
    if a.only:
        for _ in range(a.iters):
            if a.only in ("fwd", "both"):
                ops.attn_q1_fwd(x, S * D, qt, R, S, scale, drop=drop)
            if a.only in ("bwd", "both"):
                ops.attn_q1_bwd(x, S * D, qt, dc, dsig, P, R, S, scale, drop=drop)
        torch.cuda.synchronize()
        return
    new = [
        ("fwd head_expand(q0)", lambda: ops.head_expand(q0, R)),
        ("fwd gemm_nt qt [8R,512,512]", lambda: ops.gemm_nt(eq, Wt[:, D:2 * D], 8 * R, D, D)),
        ("fwd attn_q1_fwd", lambda: ops.attn_q1_fwd(x, S * D, qt, R, S, scale, drop=drop)),
        ("fwd gemm_nt o [8R,512,512]", lambda: ops.gemm_nt(c, W[2 * D:], 8 * R, D, D)),
        ("fwd head_pick(o)", lambda: ops.head_pick(go, R, sigma=sig, bias=b[2 * D:])),
        ("bwd head_expand(dao) + dsigma + sigma*dao", lambda: ops.head_expand(dao, R, bias=b[2 * D:], sigma=sig)),
        ("bwd gemm_nt dc [8R,512,512]", lambda: ops.gemm_nt(edao, Wt[:, 2 * D:], 8 * R, D, D)),
        ("bwd gemm_tn_acc dW_v [8R,512,512]", lambda: ops.gemm_tn_acc(edao, c, dW[2 * D:], 8 * R, D, D)),
        ("bwd colsum db_v", lambda: ops.colsum_acc(sdao, db[2 * D:], R, D)),
        ("bwd attn_q1_bwd", lambda: ops.attn_q1_bwd(x, S * D, qt, dc, dsig, P, R, S, scale, drop=drop)),
        ("bwd gemm_tn_acc dW_k [8R,512,512]", lambda: ops.gemm_tn_acc(eq, dqt, dW[D:2 * D], 8 * R, D, D)),
        ("bwd gemm_nt dq0 [8R,512,512]", lambda: ops.gemm_nt(dqt, W[D:2 * D], 8 * R, D, D)),
        ("bwd head_pick(dq0)", lambda: ops.head_pick(gq, R)),
    ]
    rows = [("absorbed", n, timed(f, a.iters)) for n, f in new]
    del eq, qt, c, P, go, edao, dc, dx, dqt, gq
    torch.cuda.empty_cache()

    kv = ops.gemm_nt(xf, W[D:], M, 2 * D, D, bias=b[D:])
    ao, lse = ops.attn_fwd(q0, kv, kv[:, D:], 2 * D, R, S, H, scale, save_lse=True, Sq=1, ldq=D, drop=drop)
    dq0 = torch.empty(R, D, device=dev, dtype=bf)
    dkv = torch.empty(M, 2 * D, device=dev, dtype=bf)
    bwd = lambda: ops.attn_bwd(q0, kv, kv[:, D:], 2 * D, ao, D, lse, dao, D, dq0, dkv, dkv[:, D:], 2 * D, R, S, H, scale, Sq=1, ldq=D, lddq=D, drop=drop)
    bwd()
    old = [
        ("fwd gemm_nt K|V [M,1024,512]", lambda: ops.gemm_nt(xf, W[D:], M, 2 * D, D, bias=b[D:], out=kv)),
        ("fwd attn_fwd Sq=1", lambda: ops.attn_fwd(q0, kv, kv[:, D:], 2 * D, R, S, H, scale, save_lse=True, Sq=1, ldq=D, drop=drop)),
        ("bwd attn_bwd Sq=1 (dq + dkv kernels)", bwd),
        ("bwd gemm_tn_acc dW_kv [M,1024,512]", lambda: ops.gemm_tn_acc(dkv, xf, dW[D:], M, 2 * D, D, db=db[D:])),
        ("bwd gemm_nt dX [M,512,1024]", lambda: ops.gemm_nt(dkv, Wt[:, D:], M, D, 2 * D)),
    ]
    rows += [("materialised", n, timed(f, a.iters)) for n, f in old]
    print(f"# rows {R} S {S} dropout {a.p}: median of {a.iters} launches, ms (device events)")
    for path in ("absorbed", "materialised"):
        for pth, n, t in rows:
            if pth == path:
                print(f"{path:13s} {n:45s} {t:8.3f}")
        print(f"{path:13s} {'TOTAL':45s} {sum(t for pth, _, t in rows if pth == path):8.3f}")
    fb, bb = M * D * 2, 2 * M * D * 2
    tf = next(t for _, n, t in rows if n == "fwd attn_q1_fwd")
    tb = next(t for _, n, t in rows if n == "bwd attn_q1_bwd")
    print(f"attn_q1_fwd: {fb / 1e9:.2f} GB of tokens -> {fb / tf / 1e9:.2f} TB/s;  attn_q1_bwd: {bb / 1e9:.2f} GB (read + dX) -> {bb / tb / 1e9:.2f} TB/s")


if __name__ == "__main__":
    main()
