"""The generated gfx950 assembly GEMM kernels (safevla_amd/asmgen/nt_as_gen.py) executed instruction by instruction in the lane-accurate
emulator of asmgen/amdasm.py (asynchronous loads land only at the s_waitcnt that retires them; LDS-DMA targets are poisoned until then),
against a numpy restatement of the epilogues of csrc/gemm.hip (reference layers: nn.TransformerEncoderLayer linears of
architecture/models/allenact_transformer_models/allenact_dino_transformer.py:545-552).  CPU only: this is what validates a schedule
before it is ever run on a GPU; tests/test_kernels_gpu.py compares the same kernels with the HIP kernels on hardware."""
import numpy as np
import pytest

from safevla_amd.asmgen import nt_as_gen as G
from safevla_amd.asmgen.amdasm import Emu, bf16_to_f32, f32_to_bf16_rne

def _bf16(x):
    return f32_to_bf16_rne(np.asarray(x, dtype=np.float32)).astype(np.uint16)


def _drop_keep(M, N, key, thr, row_mult):
    """keep[m, n] of svla_dropout (csrc/common.h drop_bits / drop_mix) for element index (m * row_mult) * N + n"""
    e = (np.arange(M, dtype=np.uint64)[:, None] * np.uint64(row_mult * N) + np.arange(N, dtype=np.uint64)[None, :])
    pair = e >> np.uint64(1)
    x = ((pair & np.uint64(0xffffffff)) * np.uint64(0x9E3779B1)) & np.uint64(0xffffffff)
    x ^= (((pair >> np.uint64(32)) * np.uint64(0x85EBCA77)) & np.uint64(0xffffffff))
    x ^= np.uint64(key)
    x ^= x >> np.uint64(16)
    x = ((x & np.uint64(0xffffff)) * np.uint64(0xEB352D)) & np.uint64(0xffffffff)
    x ^= x >> np.uint64(13)
    x = ((x & np.uint64(0xffffff)) * np.uint64(0x6CA68B)) & np.uint64(0xffffffff)
    x ^= x >> np.uint64(16)
    r = np.where((e & np.uint64(1)) == 0, x & np.uint64(0xffff), x >> np.uint64(16))
    return r >= np.uint64(thr)


def _bits_pack(pos, N):
    """[M, N] bool -> the blocked sign-bit layout of relu_bits_word (csrc/gemm.hip): [M/32][N/64][32 rows][8 bytes]"""
    M = pos.shape[0]
    b = np.packbits(pos.reshape(M // 32, 32, N // 64, 64), axis=-1, bitorder="little")       # [M/32, 32, N/64, 8]
    return np.ascontiguousarray(b.transpose(0, 2, 1, 3)).reshape(-1)


BF16_NAN, BF16_SENTINEL = 0x7fc0, 0x1234                       # input padding / untouched-output pattern of the padded runs
F32_SENTINEL = np.uint32(0x4b1d5eed).view(np.float32)          # the same for the fp32 dW of the tn kernel (~1.03e7: no gradient value comes near it)


def _pad_in(a, ld):
    """logical [rows, cols] input -> (the array the kernel reads: [rows, ld] with NaN in the padding columns, or ``a`` itself when ld is None; its ld)"""
    if ld is None:
        return a, a.shape[1]
    assert ld >= a.shape[1] and a.dtype == np.uint16
    buf = np.full((a.shape[0], ld), BF16_NAN, dtype=np.uint16)
    buf[:, :a.shape[1]] = a
    return buf, ld


def _pad_out(rows, cols, ld):
    """bf16 output: contiguous and NaN-filled as ever when ld is None, else [rows, ld] filled with the sentinel"""
    if ld is None:
        return np.full((rows, cols), BF16_NAN, dtype=np.uint16), cols
    assert ld >= cols
    return np.full((rows, ld), BF16_SENTINEL, dtype=np.uint16), ld


def run_kernel(flavour, M, N, grid, order=None, seed=0, alpha=1.0, key=0x1234567, p_drop=0.1, row_mult=1, gen_kw=None, nsplit=1, flags=0, K=512,
               lda=None, ldb=None, ldc=None, raw=None):
    """grid workgroups in x (panel slots) times nsplit in y (n-ranges of N / nsplit columns: the mid-M launches).  lda / ldb / ldc: padded leading
    dimensions (default: contiguous); ``raw`` (a dict) receives the output buffer as allocated, padding included."""
    g = G.NtAsGen(name="t", **dict(G.FLAVOURS[flavour], **(gen_kw or {})))
    g.build()
    assert g.K == K
    rs = np.random.RandomState(seed)
    X = _bf16(rs.standard_normal((M, K)))
    W = _bf16(rs.standard_normal((N, K)) * 0.05)
    bias = rs.standard_normal(N).astype(np.float32) if g.bias else np.zeros(N, dtype=np.float32)
    (Xm, lda), (Wm, ldb), (C, ldc) = _pad_in(X, lda), _pad_in(W, ldb), _pad_out(M, N, ldc)
    thr = int(p_drop * 65536 + 0.5)
    scale = np.float32(1.0 / (1.0 - p_drop))
    bits_in_bool = rs.rand(M, N) < 0.6
    bits = _bits_pack(bits_in_bool, N) if g.bits_in else np.zeros(M * N // 8, dtype=np.uint8)
    npanels = M // 256
    q = max(N // 256, 1)
    cmask = 0 if flags & 1 else (1 << (q.bit_length() - 1)) - 1
    for wg, wy in [(x, y) for x in range(min(grid, npanels)) for y in range(nsplit)]:
        emu = Emu(g.p, lds_bytes=g.LDS_BYTES)
        aX, aW, aB, aC, aBits = emu.alloc(Xm), emu.alloc(Wm), emu.alloc(bias), emu.alloc(C, writable=True), emu.alloc(bits, writable=True)
        ka = g.KARG.pack(A=aX, lda=lda, B=aW, ldb=ldb, bias=aB, C=aC, ldc=ldc, cmask=cmask, N=N, alpha=alpha, npanels=npanels, grid=grid, bits=aBits,
                         key=key, thr=thr, scale=float(scale), row_mult=row_mult, nr=N // nsplit, flags=flags)
        emu.run(ka, wg, order=order, wg_id_y=wy)
    acc = (bf16_to_f32(X).astype(np.float64) @ bf16_to_f32(W).astype(np.float64).T).astype(np.float32)
    out = bf16_to_f32(np.ascontiguousarray(C[:, :N]))
    if raw is not None:
        raw["C"] = C
    if g.bits_in:
        ref = np.where(bits_in_bool, acc * np.float32(alpha), np.float32(0))
    else:
        ref = acc + bias
        if g.drop:
            ref = np.where(_drop_keep(M, N, key, thr, row_mult), ref * scale, np.float32(0))
        if g.relu:
            ref = np.maximum(ref, 0)
        if g.gelu:
            from safevla_amd.asmgen import gelu_poly
            ref = gelu_poly.gelu_ref_np(ref)
    return out, ref, bits, g


def check(out, ref):
    assert not np.isnan(out).any(), f"{int(np.isnan(out).sum())} NaNs (a read of LDS-DMA data that had not landed, or an unwritten output)"
    err = np.abs(out - ref)
    tol = 2.0 ** -7 * np.abs(ref) + 2e-2          # one bf16 rounding + fp32 accumulation order
    assert (err <= tol).all(), f"{int((err > tol).sum())} elements off, max {err.max()}"


@pytest.mark.parametrize("order", [None, [3, 2, 1, 0]])
def test_nt_as_bias_two_panels_both_wave_orders(order):
    out, ref, _, _ = run_kernel("f0", 512, 512, 1, order=order)
    check(out, ref)


def test_nt_as_bias_three_workgroups_rotated_tiles():
    out, ref, _, _ = run_kernel("f0", 768, 1024, 3)
    check(out, ref)


def test_nt_as_relu_signbits():
    out, ref, bits, _ = run_kernel("f1", 512, 512, 1)
    check(out, ref)
    assert (bits == _bits_pack(out > 0, 512)).all()
    assert (out >= 0).all()


def test_nt_as_relu_dropout_signbits_matches_the_dropout_counter():
    out, ref, bits, _ = run_kernel("f1d", 512, 512, 2, row_mult=3)
    check(out, ref)
    assert (bits == _bits_pack(out > 0, 512)).all()
    kept = _drop_keep(512, 512, 0x1234567, int(0.1 * 65536 + 0.5), 3)
    assert (out[~kept] == 0).all() and 0.85 < kept.mean() < 0.95


def test_nt_as_bias_n_range_split_mid_m():
    """mid-M launches: grid (panel slots, nsplit), workgroup_id_y sweeps its own n-range of N / nsplit columns, no phases"""
    out, ref, _, _ = run_kernel("f0", 512, 512, 2, nsplit=2, flags=1)
    check(out, ref)
    out, ref, _, _ = run_kernel("f0", 256, 1024, 1, nsplit=4, flags=1, order=[2, 0, 3, 1])
    check(out, ref)


def test_nt_as_no_phase_persistent_two_panels():
    out, ref, _, _ = run_kernel("f0", 512, 256, 1, flags=1)      # one workgroup, two panels, every wave switches in the same step
    check(out, ref)


def test_nt_as_dropout_signbits_n_range_split_keeps_the_global_counter_and_bit_layout():
    out, ref, bits, _ = run_kernel("f1d", 256, 512, 1, nsplit=2, flags=1, row_mult=3)
    check(out, ref)
    assert (bits == _bits_pack(out > 0, 512)).all()
    kept = _drop_keep(256, 512, 0x1234567, int(0.1 * 65536 + 0.5), 3)
    assert (out[~kept] == 0).all()


def test_nt_as_signbit_mask_n_range_split():
    out, ref, _, _ = run_kernel("f3", 256, 512, 1, nsplit=2, flags=1, alpha=1.0 / 0.9)
    check(out, ref)


def test_nt_as_bias_n_384_does_not_read_past_the_bias():
    """N % 256 == 128: the bias table is loaded in 1-KiB chunks; the last chunk must be clamped by the descriptor"""
    out, ref, _, _ = run_kernel("f0", 256, 384, 1)
    check(out, ref)


def test_nt_as_k384_bias():
    """K = 384 (ViT-S width): 24 k-steps, 768-byte W rows fetched by 48 DMA lanes into the 1-KiB LDS pitch"""
    out, ref, _, _ = run_kernel("k384_f0", 512, 384, 1, K=384)
    check(out, ref)
    out, ref, _, _ = run_kernel("k384_f0", 256, 1152, 1, K=384, nsplit=3, flags=1, order=[3, 2, 1, 0])
    check(out, ref)


def test_nt_as_k384_gelu_flavour_evaluates_the_shared_polynomial():
    """bias + erf-GELU (the frozen ViT's fc1) as packed-fp32 Horner chains in the MFMA gaps: against the numpy restatement of asmgen/gelu_poly.py to one
    bf16 rounding, and against scipy's exact erf-GELU of the fp32 pre-activation"""
    from scipy.special import erf
    out, ref, _, _ = run_kernel("k384_f2", 256, 256, 1, K=384, flags=1)
    assert not np.isnan(out).any()
    err = np.abs(out - ref)
    assert (err <= 2.0 ** -8 * np.abs(ref) + 1e-5).all(), float(err.max())
    pre = ref        # recompute the pre-activation for the exact form
    out2, ref2, _, _ = run_kernel("k384_f0", 256, 256, 1, K=384, flags=1)      # same seed: ref2 = acc + bias
    exact = (ref2.astype(np.float64) * 0.5 * (1 + erf(ref2.astype(np.float64) / np.sqrt(2)))).astype(np.float32)
    assert np.abs(out - exact).max() <= 2.0 ** -8 * np.abs(exact).max() + 3e-5


def test_nt_as_k384_relu_signbits():
    out, ref, bits, _ = run_kernel("k384_f1", 512, 512, 1, K=384)
    check(out, ref)
    assert (bits == _bits_pack(out > 0, 512)).all() and (out >= 0).all()


def test_nt_as_signbit_mask_alpha():
    out, ref, _, _ = run_kernel("f3", 512, 512, 1, alpha=1.0 / 0.9)
    check(out, ref)
    assert (out.view(np.uint32) != 0x80000000).all()          # masked elements are +0, as in the HIP kernels


def run_tn(M, N, Kc, chunk_rows, grid, with_bias=True, seed=0, ldy=None, ldx=None, ldw=None, raw=None):
    from safevla_amd.asmgen import tn_os_gen as T
    g = T.generate()
    rs = np.random.RandomState(seed)
    dY = _bf16(rs.standard_normal((M, N)))
    X = _bf16(rs.standard_normal((M, Kc)))
    dW = rs.standard_normal((N, Kc)).astype(np.float32)
    db = rs.standard_normal(N).astype(np.float32)
    dW0, db0 = dW.copy(), db.copy()
    (dYm, ldy), (Xm, ldx) = _pad_in(dY, ldy), _pad_in(X, ldx)
    if ldw is None:
        dWm, ldw = dW, Kc
    else:      # the accumulator starts from the same values inside a sentinel-filled [N, ldw]
        dWm = np.full((N, ldw), F32_SENTINEL, dtype=np.float32)
        dWm[:, :Kc] = dW
    ntk, ntile = Kc // 256, (N // 256) * (Kc // 256)
    for wg in range(grid):
        emu = Emu(g.p, lds_bytes=g.LDS_BYTES)
        aY, aX, aW, aB = emu.alloc(dYm), emu.alloc(Xm), emu.alloc(dWm, writable=True), emu.alloc(db, writable=True)
        ka = g.KARG.pack(dY=aY, ldy=ldy, X=aX, ldx=ldx, dW=aW, ldw=ldw, db=aB if with_bias else 0, M=M, N=N, K=Kc, chunk_rows=chunk_rows,
                         ntile=ntile, ntk=ntk, grid=grid)
        emu.run(ka, wg)
    yf, xf = bf16_to_f32(dY).astype(np.float64), bf16_to_f32(X).astype(np.float64)
    if raw is not None:
        raw["dW"] = dWm
    dW = np.ascontiguousarray(dWm[:, :Kc])
    return dW, dW0 + yf.T @ xf, db, db0 + (yf.sum(0) if with_bias else 0)


def test_tn_os_two_chunks_bias_gradient():
    # one 256 x 256 tile, two row chunks (96 + 64 rows: three slots and two), bias gradient on
    dW, rW, db, rb = run_tn(160, 256, 256, 96, 2)
    assert np.abs(dW - rW).max() < 2e-3 * np.abs(rW).max()
    assert np.abs(db - rb).max() < 2e-3 * max(1.0, np.abs(rb).max())


def test_tn_os_two_k_tiles_share_the_bias_turns():
    # 256 x 512: two tiles per chunk (k-tile 0 / 1 take the bias gradient of alternate slots), five slots (ring wrap-around)
    dW, rW, db, rb = run_tn(160, 256, 512, 160, 2)
    assert np.abs(dW - rW).max() < 2e-3 * np.abs(rW).max()
    assert np.abs(db - rb).max() < 2e-3 * max(1.0, np.abs(rb).max())


def run_nt_os(flavour, M, N, Kc, grid, order=None, seed=0, lda=None, ldb=None, ldr=None, ldc=None, raw=None):
    from safevla_amd.asmgen import nt_os_gen as O
    g = O.generate(flavour)
    rs = np.random.RandomState(seed)
    X = _bf16(rs.standard_normal((M, Kc)))
    W = _bf16(rs.standard_normal((N, Kc)) * 0.05)
    bias = rs.standard_normal(N).astype(np.float32)
    R = _bf16(rs.standard_normal((M, N)))
    (Xm, lda), (Wm, ldb), (Rm, ldr), (C, ldc) = _pad_in(X, lda), _pad_in(W, ldb), _pad_in(R, ldr), _pad_out(M, N, ldc)
    ntn, ntiles = N // 256, (M // 256) * (N // 256)
    grid = min(grid, ntiles)
    for wg in range(grid):
        emu = Emu(g.p, lds_bytes=g.LDS_BYTES)
        aX, aW, aB, aR, aC = emu.alloc(Xm), emu.alloc(Wm), emu.alloc(bias), emu.alloc(Rm), emu.alloc(C, writable=True)
        ka = g.KARG.pack(A=aX, lda=lda, B=aW, ldb=ldb, bias=aB, res=aR, ldr=ldr, C=aC, ldc=ldc, M=M, N=N, K=Kc, ntn=ntn, ntiles=ntiles, grid=grid)
        emu.run(ka, wg, order=order)
    ref = (bf16_to_f32(X).astype(np.float64) @ bf16_to_f32(W).astype(np.float64).T).astype(np.float32)
    if g.bias:
        ref = ref + bias
    if g.res:
        ref = ref + bf16_to_f32(R)
    if raw is not None:
        raw["C"] = C
    return bf16_to_f32(np.ascontiguousarray(C[:, :N])), ref


@pytest.mark.parametrize("flavour,M,N,Kc,grid,order", [
    ("p", 256, 256, 384, 1, None),               # one tile, one pass of the pair loop
    ("br", 512, 512, 384, 2, [3, 2, 1, 0]),      # two tiles per workgroup (deferred stores under the next tile's K-tiles), other wave order
    ("r", 768, 256, 640, 3, None),               # three workgroups, two passes of the pair loop, residual prefetch behind the draining slabs
    ("b", 256, 512, 512, 2, None),
    ("r", 512, 1024, 384, 3, None),              # 8 tiles on 3 workgroups, 4 n-tiles per row tile: the (row tile, n-tile) cursors carry (grid % ntn = 3)
])
def test_nt_os_output_stationary_kernel(flavour, M, N, Kc, grid, order):
    """svla_nt_os_* (asmgen/nt_os_gen.py): ring of released-one-by-one units, counted waits, exposed pack + deferred stores, DOT-result hazard"""
    out, ref = run_nt_os(flavour, M, N, Kc, grid, order=order)
    check(out, ref)


def test_emulator_rejects_dot_result_read_by_another_valu_too_early():
    """The hazard the MI355X taught the builder: a DOT result is not forwarded to other VALU instructions for 3 wait states and
    the hardware does not interlock.  The emulator must refuse such a stream (and accept it with the distance kept), or the next kernel will ship the bug."""
    from safevla_amd.asmgen.amdasm import EmuError, Prog, v

    def prog(gap):
        p = Prog("t")
        p.v_mov_b32(v(1), 0x3f803f80)
        p.v_mov_b32(v(2), 0x3f803f80)
        p.v_mov_b32(v(3), 0)
        p.v_dot2c_f32_bf16(v(3), v(1), v(2))
        for _ in range(gap):
            p.v_mov_b32(v(5), 0)
        p.v_add_f32(v(4), v(3), v(3))
        p.s_endpgm()
        return p
    with pytest.raises(EmuError, match="DOT"):
        Emu(prog(2), nwaves=1).run(bytes(8), 0)
    waves = Emu(prog(3), nwaves=1).run(bytes(8), 0)
    assert (waves[0].V[4].view(np.float32) == 4.0).all()


# ------------------------------------------------------------------------------------------------ padded leading dimensions
# Every kernel forms its addresses from lda / ldb / ldc / ldr (ldy / ldx / ldw) in its own scalar and per-lane arithmetic; the product calls them with
# leading dimensions that are not the logical width (model.py: lda = ldr = ldx = S * D, row and column slices of packed qkv / weight tensors).  A padded run
# reads NaN wherever it strays into an input's padding, the emulator raises on any access outside a buffer, the output padding must keep its sentinel, and
# the logical output must equal the contiguous run of the same seed bit for bit (the operand values and the order of every sum are the same).
PAD_AS = dict(lda=181 * 512, ldb=512 + 8)       # + ldc = N + 136 per case


def _padding_untouched(buf, cols, sentinel):
    bits = np.uint16 if buf.dtype == np.uint16 else np.uint32
    pad = np.ascontiguousarray(buf[:, cols:]).view(bits)
    assert pad.size and (pad == np.asarray(sentinel, dtype=buf.dtype).view(bits)).all(), "the kernel wrote into the padding columns of its output"


def _padded_pair(runner, *args, lds, **kw):
    """the same case contiguous and padded: (padded results, contiguous results), after the checks every padded case shares"""
    cont = runner(*args, **kw)
    raw = {}
    pad = runner(*args, raw=raw, **lds, **kw)             # an access outside a buffer or a write to an input raises EmuError here
    return pad, cont, raw


def _check_padded_nt(pad, cont, raw, N):
    (out, ref), out_c = pad[:2], cont[0]
    check(out, ref)                                        # no NaN, the runner's tolerance against the reference
    _padding_untouched(raw["C"], N, np.uint16(BF16_SENTINEL))
    assert (out.view(np.uint32) == out_c.view(np.uint32)).all(), f"{int((out.view(np.uint32) != out_c.view(np.uint32)).sum())} elements differ from the contiguous run"


@pytest.mark.parametrize("order", [None, [3, 2, 1, 0]])
def test_nt_as_padded_bias_row_streaming(order):
    N = 512
    pad, cont, raw = _padded_pair(run_kernel, "f0", 512, N, 1, order=order, lds=dict(PAD_AS, ldc=N + 136))
    _check_padded_nt(pad, cont, raw, N)


def test_nt_as_padded_bias_mid_m_split():
    N = 512
    pad, cont, raw = _padded_pair(run_kernel, "f0", 256, N, 1, nsplit=2, flags=1, lds=dict(PAD_AS, ldc=N + 136))
    _check_padded_nt(pad, cont, raw, N)


def test_nt_as_padded_relu_dropout_signbits_do_not_see_ldc():
    """the dropout counter is (m * row_mult) * N + n and the sign bits are blocked by the logical N: neither may move with ldc"""
    M, N = 256, 512
    pad, cont, raw = _padded_pair(run_kernel, "f1d", M, N, 1, row_mult=3, lds=dict(PAD_AS, ldc=N + 136))
    _check_padded_nt(pad, cont, raw, N)
    out, bits = pad[0], pad[2]
    assert (bits == cont[2]).all() and (bits == _bits_pack(out > 0, N)).all()
    kept = _drop_keep(M, N, 0x1234567, int(0.1 * 65536 + 0.5), 3)
    assert (out[~kept] == 0).all() and ((out != 0) == (cont[0] != 0)).all()


def test_nt_as_padded_signbit_mask():
    N = 512
    pad, cont, raw = _padded_pair(run_kernel, "f3", 256, N, 1, nsplit=2, flags=1, alpha=1.0 / 0.9, lds=dict(PAD_AS, ldc=N + 136))
    _check_padded_nt(pad, cont, raw, N)


def test_nt_as_padded_k384_n_384_clamped_bias_chunk():
    N = 384
    pad, cont, raw = _padded_pair(run_kernel, "k384_f0", 256, N, 1, K=384, lds=dict(lda=181 * 384, ldb=384 + 8, ldc=N + 136))
    _check_padded_nt(pad, cont, raw, N)


@pytest.mark.parametrize("flavour", ["br", "r"])
def test_nt_os_padded_two_tiles_on_one_workgroup(flavour):
    """the deferred stores of tile 0 and the residual prefetch of tile 1 cross a tile boundary with ldr = 233 * 512 and ldc = N + 136"""
    N, Kc = 256, 384
    pad, cont, raw = _padded_pair(run_nt_os, flavour, 512, N, Kc, 1, lds=dict(lda=Kc + 8, ldb=Kc + 72, ldr=233 * 512, ldc=N + 136))
    _check_padded_nt(pad, cont, raw, N)


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("M,N,Kc,chunk_rows,grid", [(160, 256, 256, 96, 2), (160, 256, 512, 160, 2)])
def test_tn_os_padded(M, N, Kc, chunk_rows, grid, with_bias):
    """both shapes of the contiguous tests; the emulator runs the workgroups one after the other, so the fp32 accumulation order is fixed and the padded
    run equals the contiguous one bit for bit"""
    pad, cont, raw = _padded_pair(run_tn, M, N, Kc, chunk_rows, grid, with_bias=with_bias, lds=dict(ldy=N + 8, ldx=181 * 512, ldw=Kc + 4))
    dW, rW, db, rb = pad
    assert not np.isnan(dW).any() and not np.isnan(db).any()
    assert np.abs(dW - rW).max() < 2e-3 * np.abs(rW).max()
    assert np.abs(db - rb).max() < 2e-3 * max(1.0, np.abs(rb).max())
    _padding_untouched(raw["dW"], Kc, F32_SENTINEL)
    assert (dW.view(np.uint32) == cont[0].view(np.uint32)).all() and (db.view(np.uint32) == cont[2].view(np.uint32)).all()
    if not with_bias:
        assert (db == rb).all()                            # db = 0 in the kernarg: the bias gradient buffer is not touched
