"""Every dispatch path of svla_gemm_nt_bf16 / svla_gemm_nt_rmsa_bf16 / svla_gemm_tn_f32acc (and their fp32 twins) under padded leading dimensions.

Each kernel behind the three entry points forms its addresses from lda / ldb / ldc / ldr / ldm (ldy / ldx / ldw) in arithmetic of its own: 32-bit lane offsets,
scalar ld * 2 products, per-panel descriptor bases, pointer advances for the M % 256 tail.  The product calls them with leading dimensions that are not the
logical width (model.py: lda = ldr = ldx = S * D; row / column slices of packed qkv and weight tensors; siglip_text.py: input and output rows of one buffer).

One helper per entry point runs a call twice under the same dispatch hook -- contiguous, and with every operand padded -- and checks
  (a) the logical output is finite: the input padding columns and the spare rows behind row M hold NaN;
  (b) the output's padding columns and its 8 guard rows behind row M keep their sentinel bit pattern;
  (c) NT / rmsa / fp32: the padded result equals the contiguous one bit for bit, the ReLU sign bits too (same operand values, same order of every sum);
  (d) TN (atomic accumulation into a non-zero dW): both runs against the fp64 product with the tolerance of test_kernels_gpu.py::test_gemm_tn;
  (e) the contiguous result against a torch restatement with the tolerance of the contiguous test of the same path in test_kernels_gpu.py;
and, after either run, that ops.gemm_last_kernel() names the kernel the case is about: no case passes by falling through to another path.  The two
128-tile TN launches (gemm_tn_bf16_kernel, gemm_tn256_bf16_kernel) are not recorded by svla_gemm_last_kernel: for them the record must still show the marker
GEMM launched just before, i.e. none of the recorded TN paths was taken, which leaves the one the hook selects (gemm.hip: gemm_tn_f32acc)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_kernels_gpu import DEV, _keep_np, close, ops      # noqa: F401  (ops: fixture)

pytestmark = pytest.mark.gpu

SENT_BF16, SENT_F32 = 0x1234, 0x4B1D5EED        # untouched-output bit patterns (bf16 / fp32)
GUARD = 8                                       # sentinel rows behind an output's row M, NaN rows behind an input's
BF16, F32 = torch.bfloat16, torch.float32
SD = 181 * 512                                  # the product's lda / ldr / ldx: one [S, D] group per row (model.py: xf_stride)


def drnd(*shape, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, device=DEV, generator=g) * scale


def pad_in(t, ld, spare=GUARD):
    """logical [rows, cols] -> the same values as a view of a NaN-filled [rows + spare, ld] buffer (ld None: contiguous, no spare rows)"""
    if ld is None:
        return t.contiguous()
    rows, cols = t.shape
    assert ld >= cols
    buf = torch.full((rows + spare, ld), float("nan"), device=DEV, dtype=t.dtype)
    buf[:rows, :cols] = t
    return buf[:rows, :cols]


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def sentinel_out(rows, cols, ld, dtype, init=None):
    """[rows + GUARD, ld or cols] filled with the sentinel (the logical block with ``init`` when given: an accumulator's starting value)"""
    buf = torch.empty(rows + GUARD, ld or cols, device=DEV, dtype=dtype)
    _bits(buf).fill_(SENT_BF16 if dtype == BF16 else SENT_F32)
    if init is not None:
        buf[:rows, :cols] = init
    return buf


def untouched(buf, rows, cols, name):
    b, s = _bits(buf), (SENT_BF16 if buf.dtype == BF16 else SENT_F32)
    assert (b[rows:] == s).all(), f"{name}: guard rows behind row M were written"
    assert (b[:rows, cols:] == s).all(), f"{name}: padding columns of the output were written"


def same_bits(a, b, name):
    ne = _bits(a) != _bits(b)
    assert not ne.any(), f"{name}: {int(ne.sum())} of {ne.numel()} elements differ from the contiguous run, first at {tuple(ne.nonzero()[0].tolist())}"


def pack_bits(pos):
    """[M, N] bool -> (blocked sign-bit buffer of relu_bits_word (gemm.hip): [M/32][N/64][32 rows][8 bytes], the same-shaped mask of the bytes of rows < M)"""
    M, N = pos.shape
    MP = (M + 31) // 32 * 32
    packed = (pos.view(M, N // 8, 8).to(torch.int32) << torch.arange(8, device=DEV, dtype=torch.int32)).sum(-1).to(torch.uint8)
    pad = torch.zeros(MP, N // 8, device=DEV, dtype=torch.uint8); pad[:M] = packed
    valid = torch.zeros(MP, N // 8, device=DEV, dtype=torch.bool); valid[:M] = True
    blk = lambda t: t.view(MP // 32, 32, N // 64, 8).permute(0, 2, 1, 3).reshape(-1).contiguous()
    return blk(pad), blk(valid)


class hooked:
    """dispatch hooks of svla_gemm_force_small_tile, always restored: small = the 128-tile kernels, big = the 256-tile / assembly kernels whatever the size,
    asm_off = flag 8192 (the HIP 256-tile kernels), asm_off_2buf = + flag 128 (the 2-buffer kernels)"""
    CODES = {None: 0, "small": 1, "big": 2, "asm_off": 10 + 8192, "asm_off_2buf": 10 + 8192 + 128}

    def __init__(self, hook):
        self.code = self.CODES[hook]

    def __enter__(self):
        from safevla_amd._lib import lib
        lib().call("svla_gemm_force_small_tile", self.code)

    def __exit__(self, *exc):
        from safevla_amd._lib import lib
        lib().call("svla_gemm_force_small_tile", 0)


MARKER = ("gemm_nt_bf16_kernel", (1, 128, 64))


def launch_marker(ops):
    """a one-row GEMM of a shape no case uses: what svla_gemm_last_kernel shows for as long as no recorded path runs"""
    ops.gemm_nt(torch.zeros(1, 64, device=DEV, dtype=BF16), torch.zeros(128, 64, device=DEV, dtype=BF16), 1, 128, 64)
    assert ops.gemm_last_kernel() == MARKER


# ------------------------------------------------------------------------------------------------ NT
def nt_case(ops, M, N, K, *, expect, hook=None, lds, tol, bias=False, residual=False, relu_mask=False, act=0, out_f32=False, alpha=1.0, bits_out=False,
            bits_in=False, drop=None, b_scale=None, bias_scale=1.0, rmsa_eps=None, f32=False, ref_rows=None, asm=False):
    """``expect``: kernel name the dispatch must record (asm: with M rounded down to whole 256-row panels -- the tail rows run on the 128-tile kernel behind it
    and are compared like the others); ``lds``: the padded run's leading dimensions; ``tol``: (rtol, atol) of the path's contiguous test;
    ``ref_rows``: restrict check (e) to these rows (the 133 k-row cases: the first two panels, the last one and the tail)."""
    dt = F32 if f32 else BF16
    A = drnd(M, K, seed=1).to(dt)
    B = drnd(N, K, seed=2, scale=b_scale or 1 / math.sqrt(K)).to(dt)
    bias_t = drnd(N, seed=3, scale=bias_scale) if bias else None
    R = drnd(M, N, seed=4).to(dt) if residual else None
    Mk = drnd(M, N, seed=5).to(dt) if relu_mask else None
    pos_in = bits_t = None
    if bits_in:
        pos_in = torch.rand(M, N, device=DEV, generator=torch.Generator(device=DEV).manual_seed(6)) < 0.6
        bits_t, _ = pack_bits(pos_in)
    odt = F32 if (out_f32 or f32) else BF16

    def run(ld):
        kw = dict(act=act, alpha=alpha) if rmsa_eps is None else dict(act=act)
        Av, Bv = pad_in(A, ld.get("lda")), pad_in(B, ld.get("ldb"), spare=0)
        if bias:
            kw["bias"] = bias_t
        if residual:
            kw["residual"] = pad_in(R, ld.get("ldr"))
        if relu_mask:
            kw["relu_mask"] = pad_in(Mk, ld.get("ldm"))
        if bits_in:
            kw["relu_bits"] = bits_t
        if bits_out:
            kw["relu_bits_out"] = torch.zeros(ops.relu_bits_bytes(M, N), device=DEV, dtype=torch.uint8)
        if drop is not None:
            kw["drop"] = drop
        buf = sentinel_out(M, N, ld.get("ldc"), odt)
        out = buf[:M, :N]
        if rmsa_eps is not None:
            ops.gemm_nt_rmsa(Av, Bv, M, N, K, rmsa_eps, out=out, **kw)      # leading dimensions = the views' row strides
        else:
            if not f32:
                kw["out_f32"] = out_f32
            for k_, t_ in (("lda", Av), ("ldb", Bv), ("ldc", out), ("ldr", kw.get("residual")), ("ldm", kw.get("relu_mask"))):
                if t_ is not None:
                    kw[k_] = t_.stride(0)
                    assert kw[k_] == (ld.get(k_) or t_.shape[1])
            ops.gemm_nt(Av, Bv, M, N, K, out=out, **kw)
        torch.cuda.synchronize()
        if not f32:
            name, mnk = ops.gemm_last_kernel()
            assert name == expect and mnk == ((M // 256 * 256 if asm else M), N, K), (expect, name, mnk)
        return buf, out, kw.get("relu_bits_out")

    with hooked(hook):
        cbuf, cout, cbits = run({})
        pbuf, pout, pbits = run(lds)
    assert torch.isfinite(pout.float()).all() and torch.isfinite(cout.float()).all(), "NaN / Inf in the logical output: the kernel read padding"
    untouched(cbuf, M, N, "contiguous")
    untouched(pbuf, M, N, "padded")
    same_bits(pout, cout, expect)
    if bits_out:
        _, valid = pack_bits(torch.ones(M, N, device=DEV, dtype=torch.bool))
        assert torch.equal(pbits[valid], cbits[valid]), "ReLU sign bits differ from the contiguous run"
        want_bits, _ = pack_bits(cout.float() > 0)
        assert torch.equal(cbits[valid], want_bits[valid]), "sign bits are not (output > 0)"
    # (e) the contiguous run against torch
    rows = torch.arange(M, device=DEV) if ref_rows is None else ref_rows
    a32 = A[rows].float()
    if rmsa_eps is not None:
        a32 = a32 * torch.rsqrt((a32 * a32).mean(-1, keepdim=True) + rmsa_eps)
    v = alpha * (a32 @ B.float().t())
    if bias:
        v = v + bias_t
    if act == ops.ACT_RELU:
        v = torch.relu(v)
    elif act == ops.ACT_GELU:
        v = F.gelu(v)
    if drop is not None:
        idx = rows.cpu().numpy().astype(np.uint64)[:, None] * np.uint64(drop.c.row_mult * N) + np.arange(N, dtype=np.uint64)[None, :]
        keep = _keep_np(drop.c.seed, drop.c.stream, drop.c.p, idx).to(DEV)
        assert abs(keep.float().mean().item() - (1 - drop.c.p)) < 4 * math.sqrt(0.09 / keep.numel()) + 1e-3      # four sigma of the kept fraction
        v = torch.where(keep, v / (1 - drop.c.p), torch.zeros((), device=DEV))
        if not residual:
            assert (cout[rows].float()[~keep] == 0).all()           # every dropped element is exactly zero
    if bits_in:
        v = torch.where(pos_in[rows], v, torch.zeros((), device=DEV))
    if relu_mask:
        v = v * (Mk[rows].float() > 0)
    if residual:
        v = v + R[rows].float()
    close(cout[rows].float(), v, tol[0], tol[1], f"{expect} contiguous vs torch")


PLAIN, EPI_RES, EPI_F32, EPI_DROP, ASM = (6e-3, 6e-3), (8e-3, 4e-2), (1e-4, 1e-4), (1e-2, 2e-2), (1e-2, 2e-2)      # test_kernels_gpu.py: test_gemm_nt_plain /
# test_gemm_nt_epilogues (bias + ReLU, residual: cancellation, fp32 output) / test_gemm_nt_epilogue_dropout / the assembly-kernel tests and test_gemm_nt_rmsnorm_fused


@pytest.mark.parametrize("lda", [192 + 8, SD])
@pytest.mark.parametrize("epi", ["bias_res", "mask_res", "out_f32", "bias_res_drop181"])
@pytest.mark.parametrize("kernel", ["gemm_nt_bf16_kernel"])
def test_nt_128_tile_kernel(ops, kernel, epi, lda):
    """gemm_nt_bf16_kernel (forced): M = 300 = two full row tiles + a ragged one, every auxiliary operand padded differently"""
    M, N, K = 300, 256, 192
    lds = dict(lda=lda, ldb=K + 8, ldc=N + 8, ldr=SD, ldm=N + 72)
    kw = {"bias_res": dict(bias=True, residual=True, tol=EPI_RES), "mask_res": dict(relu_mask=True, residual=True, tol=EPI_RES),
          "out_f32": dict(bias=True, out_f32=True, alpha=0.5, tol=EPI_F32, lds=dict(lds, ldc=N + 12)),      # fp32 output: ldc % 4 is enough
          "bias_res_drop181": dict(bias=True, residual=True, drop=ops.Dropout(seed=77, stream=5, p=0.1, row_mult=181), tol=EPI_DROP)}[epi]
    nt_case(ops, M, N, K, expect=kernel, hook="small", **dict(dict(lds=lds), **kw))


@pytest.mark.parametrize("hook,expect", [("asm_off", "gemm_nt8p_bf16_kernel"), ("asm_off_2buf", "gemm_nt256k64_bf16_kernel")])
@pytest.mark.parametrize("epi", ["bias_relu_bits_out", "bias_res", "mask_res", "bits_in"])
def test_nt_256_tile_hip_kernels(ops, epi, hook, expect):
    """the 8-phase and the 2-buffer kernel at 41 x 4 = 164 tiles (just over the 160-tile threshold of the dispatch), last row tile 77 rows"""
    M, N, K = 256 * 40 + 77, 1024, 192
    kw = {"bias_relu_bits_out": dict(bias=True, act=ops.ACT_RELU, bits_out=True, tol=PLAIN), "bias_res": dict(bias=True, residual=True, tol=EPI_RES),
          "mask_res": dict(relu_mask=True, residual=True, tol=EPI_RES), "bits_in": dict(bits_in=True, tol=PLAIN)}[epi]
    nt_case(ops, M, N, K, expect=expect, hook=hook, lds=dict(lda=K + 64, ldb=K + 8, ldc=N + 136, ldr=N + 8, ldm=N + 72), **kw)


def _as_kw(ops, kernel):
    flavour = kernel.rsplit("_", 1)[1]
    return {"f0": dict(bias=True), "f1": dict(bias=True, act=ops.ACT_RELU, bits_out=True),
            "f1d": dict(bias=True, act=ops.ACT_RELU, bits_out=True, drop=ops.Dropout(seed=99, stream=3, p=0.1, row_mult=3)),
            "f3": dict(bits_in=True, alpha=1 / 0.9), "f2": dict(bias=True, act=ops.ACT_GELU)}[flavour]


@pytest.mark.parametrize("N", [512, 1536])
@pytest.mark.parametrize("kernel", ["svla_nt_as_f0", "svla_nt_as_f1", "svla_nt_as_f1d", "svla_nt_as_f3"])
def test_nt_a_stationary_mid_m(ops, kernel, N):
    """svla_nt_as_* in the mid-M launch (grid = panel slots x n-ranges), forced at three panels + a 5-row tail on the 128-tile kernel; lda = the product's S * D"""
    M, K = 256 * 3 + 5, 512
    nt_case(ops, M, N, K, expect=kernel, hook="big", asm=True, lds=dict(lda=SD, ldb=K + 8, ldc=N + 136), tol=ASM, b_scale=0.05,
            bias_scale=0.5, **_as_kw(ops, kernel))


@pytest.mark.parametrize("N", [384, 1152])
@pytest.mark.parametrize("kernel", ["svla_nt_as_k384_f0", "svla_nt_as_k384_f2"])
def test_nt_a_stationary_k384(ops, kernel, N):
    """the K = 384 flavours (768-byte W rows in the 1-KiB LDS pitch); N = 384: the clamped last bias chunk"""
    M, K = 256 * 3 + 5, 384
    nt_case(ops, M, N, K, expect=kernel, hook="big", asm=True, lds=dict(lda=181 * 384, ldb=K + 8, ldc=N + 136), tol=ASM, b_scale=0.05,
            bias_scale=0.5, **_as_kw(ops, kernel))


@pytest.mark.parametrize("kernel", ["svla_nt_as_f0", "svla_nt_as_f1d"])
def test_nt_a_stationary_row_streaming(ops, kernel):
    """the persistent row-streaming launch (>= 2 panels per CU, phases) under normal dispatch; the torch restatement on the first two panels, the last
    panel and the tail (all rows are compared with the contiguous run)"""
    M, N, K = 256 * 520 + 77, 512, 512
    rows = torch.cat([torch.arange(0, 512, device=DEV), torch.arange(M - 77 - 256, M, device=DEV)])
    nt_case(ops, M, N, K, expect=kernel, asm=True, lds=dict(lda=K + 64, ldc=N + 136), tol=ASM, b_scale=0.05, bias_scale=0.5, ref_rows=rows,
            **_as_kw(ops, kernel))


@pytest.mark.parametrize("K,kernel", [(512, "svla_nt_os_br"), (512, "svla_nt_os_r"), (1536, "svla_nt_os_br"), (1536, "svla_nt_os_r"), (1536, "svla_nt_os_b")])
def test_nt_output_stationary(ops, K, kernel):
    """svla_nt_os_* forced at 3 x 2 tiles (deferred stores and the residual prefetch cross tile boundaries on every workgroup that holds two), 5-row tail;
    ldr = 233 * 512: a residual read out of a [233, 512] group per row"""
    M, N = 256 * 3 + 5, 512
    flavour = kernel.rsplit("_", 1)[1]
    nt_case(ops, M, N, K, expect=kernel, hook="big", asm=True, lds=dict(lda=K + 8, ldb=K + 72, ldr=233 * 512, ldc=N + 136), tol=ASM,
            b_scale=0.05, bias_scale=0.5, bias="b" in flavour, residual="r" in flavour)


def test_nt_rmsnorm_fused(ops):
    """svla_gemm_nt_rmsa_bf16 (128-tile kernel, row statistics out of the A fragments: a NaN in A's padding would poison the whole row)"""
    M, N, K = 130, 512, 512
    nt_case(ops, M, N, K, expect="gemm_nt_bf16_kernel", lds=dict(lda=K + 8, ldb=K + 8, ldr=N + 72, ldc=N + 136), tol=(1e-2, 2e-2), b_scale=0.05, bias=True,
            residual=True, rmsa_eps=1e-5)


def _f32_tol(K):
    # fp32 FMA chain of K terms: each of the K roundings is at most 2^-24 of a partial sum bounded by sum |a b| (operands ~N(0, 1) x N(0, 1 / K): each
    # |output| and sum |a b| are O(1), the latter ~0.64 sqrt(K) at most ~6 here) -> K * 2^-24 * 6 absolute, plus one rounding of the result
    return (2.0 ** -23, K * 2.0 ** -24 * 6)


def test_nt_fp32_twin(ops):
    """gemm_nt on fp32 operands (svla_gemm_f32: the verification mode's GEMM), all five leading dimensions padded, ragged in M (70 = 64 + 6)"""
    M, N, K = 70, 128, 64
    nt_case(ops, M, N, K, expect=None, f32=True, lds=dict(lda=K + 4, ldb=K + 12, ldc=N + 4, ldr=N + 20, ldm=N + 8), tol=_f32_tol(K), bias=True, residual=True,
            relu_mask=True)


# ------------------------------------------------------------------------------------------------ TN
def tn_case(ops, M, N, K, *, expect, recorded=True, hook=None, lds, with_db=True, mnk=None):
    """``recorded`` False: a launch svla_gemm_last_kernel does not record -- the marker must survive the call (see the module docstring)"""
    dt = BF16
    dY, X = drnd(M, N, seed=1).to(dt), drnd(M, K, seed=2).to(dt)
    w0, b0 = drnd(N, K, seed=3), drnd(N, seed=4)
    want_w = w0.double() + dY.double().t() @ X.double()
    want_b = b0.double() + dY.double().sum(0)
    res = []
    with hooked(hook):
        for ld in ({}, lds):
            wbuf = sentinel_out(N, K, ld.get("ldw"), F32, init=w0)
            bbuf = sentinel_out(1, N, None, F32, init=b0[None])
            dW, db = wbuf[:N, :K], bbuf[0]
            Yv, Xv = pad_in(dY, ld.get("ldy")), pad_in(X, ld.get("ldx"))
            launch_marker(ops)
            ops.gemm_tn_acc(Yv, Xv, dW, M, N, K, ldy=Yv.stride(0), ldx=Xv.stride(0), ldw=dW.stride(0), db=db if with_db else None)
            torch.cuda.synchronize()
            assert ops.gemm_last_kernel() == ((expect, mnk or (M, N, K)) if recorded else MARKER), (expect, ops.gemm_last_kernel())
            res.append((wbuf, bbuf, dW, db))
    for (wbuf, bbuf, dW, db), name in zip(res, ("contiguous", "padded")):
        assert torch.isfinite(dW).all() and torch.isfinite(db).all(), f"{name}: NaN / Inf in the gradient: the kernel read padding"
        untouched(wbuf, N, K, name + " dW")
        untouched(bbuf, 1, N, name + " db")
        close(dW, want_w, 2e-4, 2e-4 * math.sqrt(M), name + " dW")
        if with_db:
            close(db, want_b, 2e-4, 2e-4 * math.sqrt(M), name + " db")
        else:
            assert torch.equal(db, b0), name + ": db written without being asked for"


TN_LDS = dict(ldy=512 + 8, ldx=SD, ldw=512 + 4)


@pytest.mark.parametrize("kernel", ["gemm_tn_bf16_kernel+svla_colsum_bf16"])
def test_tn_128_tile_kernel_and_colsum(ops, kernel):
    """gemm_tn_bf16_kernel (forced; not recorded) + svla_colsum_bf16 for the bias gradient; M = 1000: ragged in the 64-row reduction tile"""
    tn_case(ops, 1000, 128, 128, expect=kernel, recorded=False, hook="small", lds=dict(ldy=128 + 8, ldx=128 + 72, ldw=128 + 4))


@pytest.mark.parametrize("with_db", [True, False], ids=["db", "no_db"])
@pytest.mark.parametrize("kernel", ["svla_tn_os"])
def test_tn_output_stationary_assembly(ops, kernel, with_db):
    """svla_tn_os forced at five 64-row groups; ldx = the product's S * D"""
    tn_case(ops, 320, 512, 512, expect=kernel, hook="big", lds=TN_LDS, with_db=with_db)


@pytest.mark.parametrize("kernel", ["svla_tn_os+gemm_tn_bf16_kernel"])
def test_tn_forced_ragged_split(ops, kernel):
    """M = 327 under the force-big hook: 320 rows on svla_tn_os, 7 on the 128-tile kernel (+ column sum) behind pointers advanced by mb * ldy / mb * ldx"""
    tn_case(ops, 327, 512, 512, expect=kernel.split("+")[0], mnk=(320, 512, 512), hook="big", lds=TN_LDS)      # the record keeps the first launch


@pytest.mark.parametrize("hook,expect,recorded", [("asm_off", "gemm_tn8p_bf16_kernel", True), ("asm_off_2buf", "gemm_tn256_bf16_kernel", False)])
def test_tn_256_tile_hip_kernels(ops, hook, expect, recorded):
    """gemm_tn8p_bf16_kernel / gemm_tn256_bf16_kernel (the latter not recorded).  The flags that switch the assembly off also clear the force-big hook
    (svla_gemm_force_small_tile keeps one or the other), so the 256-tile path must be reached by size: M = 16384, its threshold.  With ldx = S * D that
    is the X the product hands over at 64 envs x 256 steps, 3 GB end to end: byte offsets beyond 2^31."""
    tn_case(ops, 16384, 512, 512, expect=expect, recorded=recorded, hook=hook, lds=TN_LDS)


def test_colsum_alone(ops):
    """svla_colsum_bf16 with row_stride = 181 (token 0 of every [S, D] group) and a padded ldy: atomic accumulation, so both runs against the sum
    (tolerance of test_colsum); every row it must not read holds NaN"""
    M, N, rs = 50, 512, 181
    dY = drnd(M, N, seed=1).bfloat16()
    want = 1 + dY.double().sum(0)
    for ldy in (N, N + 8):
        buf = torch.full((M * rs, ldy), float("nan"), device=DEV, dtype=BF16)
        buf[::rs, :N] = dY
        bbuf = sentinel_out(1, N, None, F32, init=torch.ones(1, N, device=DEV))
        ops.colsum_acc(buf, bbuf[0], M, N, ldy=ldy, row_stride=rs)
        torch.cuda.synchronize()
        untouched(bbuf, 1, N, f"colsum ldy={ldy}")
        close(bbuf[0], want, 1e-4, 1e-3, f"colsum ldy={ldy}")


def test_tn_fp32_twin(ops):
    """gemm_tn_acc on fp32 operands (svla_gemm_f32 with transposed strides, accumulate; svla_colsum_f32), every leading dimension padded"""
    M, N, K = 70, 128, 128
    dY, X = drnd(M, N, seed=1), drnd(M, K, seed=2)
    w0, b0 = drnd(N, K, seed=3), drnd(N, seed=4)
    want_w, want_b = w0.double() + dY.double().t() @ X.double(), b0.double() + dY.double().sum(0)
    # M-term fp32 chains on N(0, 1) operands: M roundings of at most 2^-24 of a partial sum bounded by sum |dy x| (~0.64 M, at most ~1.5 M in the tail)
    atol = M * 2.0 ** -24 * 1.5 * M
    res = []
    for ld in ({}, dict(ldy=N + 4, ldx=K + 12, ldw=K + 20)):
        wbuf, bbuf = sentinel_out(N, K, ld.get("ldw"), F32, init=w0), sentinel_out(1, N, None, F32, init=b0[None])
        Yv, Xv = pad_in(dY, ld.get("ldy")), pad_in(X, ld.get("ldx"))
        ops.gemm_tn_acc(Yv, Xv, wbuf[:N, :K], M, N, K, ldy=Yv.stride(0), ldx=Xv.stride(0), ldw=wbuf.stride(0), db=bbuf[0])
        torch.cuda.synchronize()
        untouched(wbuf, N, K, "fp32 dW"); untouched(bbuf, 1, N, "fp32 db")
        res.append((wbuf[:N, :K], bbuf[0]))
    close(res[0][0], want_w, 2.0 ** -23, atol, "fp32 dW"); close(res[0][1], want_b, 2.0 ** -23, atol, "fp32 db")
    same_bits(res[1][0], res[0][0], "fp32 dW"); same_bits(res[1][1], res[0][1], "fp32 db")        # one thread per output, fixed order: bit for bit


# ------------------------------------------------------------------------------------------------ the product's own calls
@pytest.mark.parametrize("R", [5, 256 * 3 + 5])
def test_product_pruned_last_layer_calls(ops, R):
    """model.py, the pruned last fusion layer at S = 181, D = 512, plain dispatch: the query projection reads row 0 of every [S, D] group (lda = S * D); out_proj
    adds the residual from there (ldr = S * D) under a dropout whose counter strides by S rows; the Q weight gradient reads X with ldx = S * D (the absorbed
    and the materialised branch make the same call).  Contiguous = the same rows gathered first."""
    D, S = 512, 181
    nt_case(ops, R, D, D, expect="gemm_nt_bf16_kernel", lds=dict(lda=S * D), tol=PLAIN, bias=True)                                    # q0 = xf[::S] Wq^T + b
    nt_case(ops, R, D, D, expect="gemm_nt_bf16_kernel", lds=dict(ldr=S * D), tol=EPI_DROP, bias=True, residual=True, b_scale=0.1, bias_scale=0.1,
            drop=ops.Dropout(seed=77, stream=1, p=0.1, row_mult=S))                                                                    # h1 = drop(ao Wo^T + b) + xf[::S]
    tn_case(ops, R, D, D, expect="gemm_tn_bf16_kernel", recorded=False, lds=dict(ldx=S * D))                                                                           # dWq += dq0^T xf[::S]


@pytest.mark.parametrize("same_buffer_input", [True, False])
def test_product_siglip_text_pooled_projection(ops, same_buffer_input):
    """siglip_text.py: the pooled projection of the last token, written into the [U, Lo, W] token buffer it (Lo = L + 1: lda = ldc = (L + 1) W) or a copy of
    it (Lo = L: ldc = L W) was read from; every row the call must not touch keeps its bits"""
    U, L, W = 3, 4, 768
    Lo = L + 1 if same_buffer_input else L
    tokens = drnd(U, Lo, W, seed=1).bfloat16()
    proj, bias = drnd(W, W, seed=2, scale=1 / math.sqrt(W)).bfloat16(), drnd(W, seed=3)
    last = tokens[:, L - 1].contiguous()
    want = ops.gemm_nt(last, proj, U, W, W, bias=bias)                          # contiguous in, contiguous out
    torch.cuda.synchronize()
    assert ops.gemm_last_kernel() == ("gemm_nt_bf16_kernel", (U, W, W))
    close(want.float(), last.float() @ proj.float().t() + bias, *PLAIN, "pooled projection vs torch")
    out = tokens.clone()
    if same_buffer_input:
        ops.gemm_nt(out[:, L - 1], proj, U, W, W, bias=bias, out=out[:, L], lda=(L + 1) * W, ldc=(L + 1) * W)
    else:
        ops.gemm_nt(last, proj, U, W, W, bias=bias, out=out[:, L - 1], ldc=L * W)
    torch.cuda.synchronize()
    assert ops.gemm_last_kernel() == ("gemm_nt_bf16_kernel", (U, W, W))
    dst = L if same_buffer_input else L - 1
    same_bits(out[:, dst], want, "pooled rows")
    keep = [t for t in range(Lo) if t != dst]
    same_bits(out[:, keep], tokens[:, keep], "rows the call must not touch")
