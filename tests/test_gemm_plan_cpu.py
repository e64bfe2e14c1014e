"""Which kernel carries a bf16 GEMM, and with what launch geometry: nt_plan / tn_plan of safevla_amd/csrc/gemm_host.h through the read-only entry points
svla_gemm_nt_plan / svla_gemm_tn_plan (include/svla.h), which touch no HIP API -- no GPU needed.

The tables are LITERAL: every row was derived by hand from the dispatch rules as they stood in gemm.hip before the planner existed (nt_as_try, nt_os_try, the
256-tile condition of svla_gemm_nt_bf16, gemm_tn_f32acc), at 256 compute units with every assembly kernel present, for the shapes the product and the GPU
tests use.  Never regenerate an expected value by running the planner.  Arithmetic of the rules, for the mid-M rows (A-stationary kernels, fewer than 2 n_cu = 512
256-row panels):
    asm  = min over the divisors d of N/128 of  rounds * (N/64/d + 5)  n-steps, slots = panels if panels * d <= n_cu else n_cu // d, rounds = ceil(panels / slots),
           times 2.76 us * K/512, plus 15 us when M % 256 != 0;
    tile = ceil(ceil(M/256) * ceil(N/256) / n_cu) * (6.2 + 11.6 K/512) us;       taken when asm <= 0.95 tile, or always under force 2.
"""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AS, OS, P8, B2, T128 = range(5)                 # NtPlan::path
TN_OS, TN_8P, TN_2BUF, TN_128 = range(4)        # TnPart::path
BIAS, RES, MASK, BITS_IN, BITS_OUT = 1, 2, 4, 8, 16
RELU, GELU = 1, 2
NT8P, NT2B, NT128 = "gemm_nt8p_bf16_kernel", "gemm_nt256k64_bf16_kernel", "gemm_nt_bf16_kernel"
TN8P, TN2B, TN128 = "gemm_tn8p_bf16_kernel", "gemm_tn256_bf16_kernel", "gemm_tn_bf16_kernel"


@pytest.fixture(scope="module")
def cdll():
    from safevla_amd import build
    lib = ctypes.CDLL(build.build())
    i, p = ctypes.c_int, ctypes.c_void_p
    lib.svla_gemm_nt_plan.argtypes, lib.svla_gemm_nt_plan.restype = [i, i, i, i, i, i, ctypes.c_float, i, i, i, p, i, p], i
    lib.svla_gemm_tn_plan.argtypes, lib.svla_gemm_tn_plan.restype = [i, i, i, i, i, i, p, i, p], i
    lib.svla_gemm_force_small_tile.argtypes, lib.svla_gemm_force_small_tile.restype = [i], i
    yield lib
    lib.svla_gemm_force_small_tile(0)


def _query(cdll, fn, n_out, hook, *scalars):
    buf, out = ctypes.create_string_buffer(96), (ctypes.c_int * n_out)()
    cdll.svla_gemm_force_small_tile(hook)      # without a device it reports the failed device initialisation (-1) and sets the hook all the same
    try:
        rc = fn(*scalars, ctypes.cast(buf, ctypes.c_void_p), 96, ctypes.cast(out, ctypes.c_void_p))
    finally:
        cdll.svla_gemm_force_small_tile(0)
    assert rc == 0, rc
    return (buf.value.decode(), *out)


def nt(cdll, M, N, K, epi=0, act=0, out_f32=0, alpha=1.0, drop=0, row_mult=1, hook=0, n_cu=256):
    return _query(cdll, cdll.svla_gemm_nt_plan, 10, hook, M, N, K, act, out_f32, epi, alpha, drop, row_mult, n_cu)


def tn(cdll, M, N, K, db=1, det=0, hook=0, n_cu=256):
    return _query(cdll, cdll.svla_gemm_tn_plan, 12, hook, M, N, K, db, det, n_cu)


F1 = dict(epi=BIAS | BITS_OUT, act=RELU)
FORCE_BIG, FORCE_SMALL, ASM_OFF, ASM_OFF_2BUF = 2, 1, 10 + 8192, 10 + 8192 + 128
# (M, N, K, call) -> (kernel, path, main rows, tail rows, grid_x, grid_y, nr, flags, cmask, log extra bytes / row, log joinable)
NT = [
    # ---- the update's row-streaming shapes: 2896 panels >= 512, one persistent workgroup per CU, cmask + 1 = largest power of two <= N / 256
    ((741376, 512, 512, dict(epi=BIAS)),                                    ("svla_nt_as_f0", AS, 741376, 0, 256, 1, 512, 0, 1, 0, 1)),
    ((741476, 2048, 512, dict(F1, drop=1)),                                 ("svla_nt_as_f1d", AS, 741376, 100, 256, 1, 2048, 0, 7, 256, 1)),
    ((741376, 2048, 512, dict(epi=BITS_IN)),                                ("svla_nt_as_f3", AS, 741376, 0, 256, 1, 2048, 0, 7, 256, 1)),
    ((741376, 512, 2048, dict(epi=BITS_IN)),                                (NT8P, P8, 741376, 0, 256, 1, 0, 0, 0, 64, 1)),           # K = 2048: no A-stationary kernel; sign bits: no output-stationary one
    ((741376, 512, 2048, dict(epi=BIAS | RES)),                             ("svla_nt_os_br", OS, 741376, 0, 256, 1, 0, 0, 0, 1024, 1)),
    ((741376, 512, 2048, dict(epi=BIAS | RES, drop=1)),                     (NT8P, P8, 741376, 0, 256, 1, 0, 0, 0, 1024, 1)),         # dropout: no output-stationary kernel
    ((741376, 512, 512, dict(epi=BIAS | RES)),                              ("svla_nt_os_br", OS, 741376, 0, 256, 1, 0, 0, 0, 1024, 1)),
    ((131136, 512, 1536, dict(epi=RES)),                                    ("svla_nt_os_r", OS, 131072, 64, 256, 1, 0, 0, 0, 1024, 1)),   # 512 x 2 = 1024 tiles: the threshold itself
    # ---- mid-M.  45 panels, N = 1536 (12 x 128, 24 steps): d = 4 -> 180 <= 256 slots, 1 round x (6 + 5) = 11 steps (d = 3: 13, d = 6: 42 slots, 2 x 9 = 18)
    #      asm 11 x 2.76 = 30.4 us; tile ceil(45 x 6 / 256) = 2 rounds x 17.8 = 35.6 us, x 0.95 = 33.8: taken
    ((11520, 1536, 512, dict(epi=BIAS)),                                    ("svla_nt_as_f0", AS, 11520, 0, 45, 4, 384, 1, 0, 0, 1)),
    #      N = 512 (8 steps): d = 4 -> 1 x (2 + 5) = 7 steps = 19.3 us; tile 1 round (90 tiles) = 17.8 us: refused; 90 < 1024 and < 160 tiles: the 128-tile kernel, 90 x 4 workgroups
    ((11520, 512, 512, dict()),                                             (NT128, T128, 11520, 0, 360, 1, 0, 0, 0, 0, 0)),
    #      N = 2048 (32 steps): d = 4 -> 8 + 5 = 13 steps (d = 8: 32 slots, 2 x 9 = 18) = 35.9 us; tile 2 rounds (360 tiles) = 35.6 us: refused
    ((11520, 2048, 512, dict(F1)),                                          (NT8P, P8, 11520, 0, 256, 1, 0, 0, 0, 256, 1)),
    #      233 panels, N = 512: d = 1 -> 233 slots, 8 + 5 = 13 steps (d = 2: 128 slots, 2 x 9 = 18) = 35.9 us; tile 2 rounds (466 tiles) = 35.6 us: refused
    ((59648, 512, 512, dict(epi=BIAS)),                                     (NT8P, P8, 59648, 0, 256, 1, 0, 0, 0, 0, 1)),
    ((59648, 512, 512, dict(epi=BIAS, hook=FORCE_BIG)),                     ("svla_nt_as_f0", AS, 59648, 0, 233, 1, 512, 1, 0, 0, 1)),
    #      N = 1536: d = 1 -> 24 + 5 = 29 steps (d = 2: 128 slots, 2 x 17 = 34) = 80.0 + 15 (tail) = 95.0 us; tile ceil(234 x 6 / 256) = 6 rounds = 106.8 us, x 0.95 = 101.5: taken
    ((59653, 1536, 512, dict(epi=BIAS)),                                    ("svla_nt_as_f0", AS, 59648, 5, 233, 1, 1536, 1, 0, 0, 1)),
    #      300 panels, N = 2048: d = 2 -> 128 slots, 3 rounds x (16 + 5) = 63 steps (d = 1: 2 x 37 = 74, d = 4: 5 x 13 = 65) = 173.9 us; tile ceil(2400 / 256) = 10 rounds = 178 us,
    #      x 0.95 = 169.1: refused; 2400 >= 1024 tiles: output-stationary
    ((76800, 2048, 512, dict(epi=BIAS)),                                    ("svla_nt_os_b", OS, 76800, 0, 256, 1, 0, 0, 0, 0, 1)),
    ((76800, 2048, 512, dict(F1, hook=FORCE_BIG)),                          ("svla_nt_as_f1", AS, 76800, 0, 128, 2, 1024, 1, 0, 256, 1)),
    # ---- K = 384 (steps cost 0.75 x 2.76 = 2.07 us, tile rounds 6.2 + 8.7 = 14.9 us), 216 panels
    #      N = 384 (3 x 128, 6 steps): d = 1 -> 6 + 5 = 11 steps (d = 3: 85 slots, 3 x 7 = 21) = 22.8 us; tile ceil(216 x 2 / 256) = 2 rounds = 29.8, x 0.95 = 28.3: taken
    ((55296, 384, 384, dict(epi=BIAS)),                                     ("svla_nt_as_k384_f0", AS, 55296, 0, 216, 1, 384, 1, 0, 0, 1)),
    #      N = 1536: d = 1 -> 29 steps = 60.0 us; tile ceil(1296 / 256) = 6 rounds = 89.4, x 0.95 = 84.9: taken
    ((55296, 1536, 384, dict(epi=BIAS, act=GELU)),                          ("svla_nt_as_k384_f2", AS, 55296, 0, 216, 1, 1536, 1, 0, 0, 1)),
    #      N = 1152 (9 x 128, 18 steps): d = 1 -> 23 steps (d = 3: 85 slots, 3 x 11 = 33) = 47.6 us; tile ceil(216 x 5 / 256) = 5 rounds = 74.5, x 0.95 = 70.8: taken
    ((55296, 1152, 384, dict(epi=BIAS)),                                    ("svla_nt_as_k384_f0", AS, 55296, 0, 216, 1, 1152, 1, 0, 0, 1)),
    ((55296, 384, 1536, dict(epi=BIAS | RES)),                              (NT8P, P8, 55296, 0, 256, 1, 0, 0, 0, 768, 1)),           # N % 256 != 0: no output-stationary kernel; half last n-tile
    #      160 panels, N = 640 (5 x 128, 10 steps): d = 1 -> 15 steps = 41.4 us; tile ceil(160 x 3 / 256) = 2 rounds = 35.6: refused
    ((40960, 640, 512, dict(epi=BIAS)),                                     (NT8P, P8, 40960, 0, 256, 1, 0, 0, 0, 0, 1)),
    # ---- epilogues no assembly kernel has
    ((40960, 512, 512, dict(epi=MASK)),                                     (NT8P, P8, 40960, 0, 256, 1, 0, 0, 0, 1024, 1)),
    ((262144, 512, 512, dict(epi=BIAS, alpha=0.5)),                         (NT8P, P8, 262144, 0, 256, 1, 0, 0, 0, 0, 1)),
    ((4096, 512, 512, dict(out_f32=1)),                                     (NT128, T128, 4096, 0, 128, 1, 0, 0, 0, 0, 0)),
    # ---- small M.  2085 rows = 8 panels (the floor): d = 4 -> 7 steps = 19.3 + 15 = 34.3 us; tile 1 round = 17.8: refused; 17 row tiles x 4
    ((2085, 512, 512, dict(epi=BIAS)),                                      (NT128, T128, 2085, 0, 68, 1, 0, 0, 0, 0, 0)),
    ((2085, 512, 512, dict(epi=BIAS, hook=FORCE_BIG)),                      ("svla_nt_as_f0", AS, 2048, 37, 8, 4, 128, 1, 0, 0, 1)),
    ((512, 512, 512, dict(epi=BIAS, hook=FORCE_BIG)),                       ("svla_nt_as_f0", AS, 512, 0, 2, 4, 128, 1, 0, 0, 1)),
    ((100, 512, 512, dict(epi=BIAS, hook=FORCE_BIG)),                       (NT8P, P8, 100, 0, 8, 1, 0, 0, 0, 0, 1)),                 # no whole panel; 2 tiles: one workgroup per XCD
    ((2048, 512, 512, dict(epi=BIAS, hook=FORCE_SMALL)),                    (NT128, T128, 2048, 0, 64, 1, 0, 0, 0, 0, 0)),
    ((741376, 512, 512, dict(epi=BIAS, hook=ASM_OFF)),                      (NT8P, P8, 741376, 0, 256, 1, 0, 0, 0, 0, 1)),
    ((741376, 512, 512, dict(epi=BIAS, hook=ASM_OFF_2BUF)),                 (NT2B, B2, 741376, 0, 256, 1, 0, 0, 0, 0, 1)),
    ((131072, 512, 512, dict(epi=BIAS, n_cu=64)),                           ("svla_nt_as_f0", AS, 131072, 0, 64, 1, 512, 0, 1, 0, 1)),  # 512 panels >= 2 x 64: row-streaming
]
NONE = (0, 0, 0, 0, 0, 0)      # no tail part
# (M, N, K, call) -> (kernel[+tail kernel], main: path, rows, chunk_rows, grid, colsum in front, recorded, tail: the same)
TN = [
    ((741376, 512, 512, dict()),                  ("svla_tn_os", TN_OS, 741376, 11584, 256, 0, 1, *NONE)),       # 4 tiles x 64 chunks of 741376 / 64 rows
    ((741376, 2048, 512, dict()),                 ("svla_tn_os", TN_OS, 741376, 46336, 256, 0, 1, *NONE)),       # 16 tiles x 16 chunks
    ((741376, 512, 512, dict(det=1)),             (TN8P, TN_8P, 741376, 11584, 256, 0, 1, *NONE)),
    ((741376, 512, 512, dict(hook=ASM_OFF)),      (TN8P, TN_8P, 741376, 11584, 256, 0, 1, *NONE)),
    ((741376, 512, 512, dict(hook=ASM_OFF_2BUF)), (TN2B, TN_2BUF, 741376, 11584, 256, 0, 0, *NONE)),
    ((8192, 512, 512, dict()),                    (TN128, TN_128, 8192, 256, 512, 1, 0, *NONE)),                 # 8 k rows, N K < 512 k; 16 tiles x 32 chunks of the 256-row floor
    ((8192, 2048, 512, dict()),                   ("svla_tn_os", TN_OS, 8192, 512, 256, 0, 1, *NONE)),
    ((16384, 512, 512, dict(db=0)),               ("svla_tn_os", TN_OS, 16384, 256, 256, 0, 1, *NONE)),
    ((16400, 512, 512, dict()),                   (TN128, TN_128, 16400, 256, 1040, 1, 0, *NONE)),               # M % 64 != 0; 16 tiles x 65 chunks
    ((1000, 512, 512, dict(hook=FORCE_BIG)),      ("svla_tn_os+" + TN128, TN_OS, 960, 64, 60, 0, 1, TN_128, 40, 256, 16, 1, 0)),
    ((64, 512, 512, dict(hook=FORCE_BIG)),        ("svla_tn_os", TN_OS, 64, 64, 4, 0, 1, *NONE)),
    ((741376, 384, 384, dict()),                  (TN128, TN_128, 741376, 3264, 2052, 1, 0, *NONE)),             # 9 tiles: 228 chunks of ceil(741376 / 228) -> 51 x 64 rows
    ((4096, 1536, 512, dict(hook=FORCE_SMALL)),   (TN128, TN_128, 4096, 256, 768, 1, 0, *NONE)),                 # 48 tiles x 16 chunks
]


def _id(row):
    (M, N, K, kw), _ = row
    return f"{M}x{N}x{K}" + "".join(f",{k}={v}" for k, v in kw.items())


@pytest.mark.parametrize("row", NT, ids=_id)
def test_nt_plan(cdll, row):
    (M, N, K, kw), want = row
    assert nt(cdll, M, N, K, **kw) == want


@pytest.mark.parametrize("row", TN, ids=_id)
def test_tn_plan(cdll, row):
    (M, N, K, kw), want = row
    assert tn(cdll, M, N, K, **kw) == want


def test_32_bit_guards_refuse_the_assembly_kernels(cdll):
    """the dropout counter of svla_nt_as_f1d counts element pairs of the logical [M row_mult, N] tensor in 32 bits; the sign-bit offset of a panel is 32-bit
    scalar arithmetic (bytes: M N / 8) in every A-stationary kernel that reads or writes the bits"""
    M, N = 741376, 2048
    assert M * 5 * N // 2 < 2 ** 32 - 1 <= M * 6 * N // 2
    assert nt(cdll, M, N, 512, drop=1, row_mult=5, **F1)[:2] == ("svla_nt_as_f1d", AS)
    assert nt(cdll, M, N, 512, drop=1, row_mult=6, **F1)[:2] == (NT8P, P8)
    M, N = 2 ** 23, 4096
    assert (M - 256) * N // 8 < 2 ** 32 - 1 <= M * N // 8
    assert nt(cdll, M - 256, N, 512, epi=BITS_IN)[:2] == ("svla_nt_as_f3", AS)
    assert nt(cdll, M, N, 512, epi=BITS_IN)[:2] == (NT8P, P8)
    assert nt(cdll, M - 256, N, 512, **F1)[:2] == ("svla_nt_as_f1", AS)
    assert nt(cdll, M, N, 512, **F1)[:2] == (NT8P, P8)
    assert nt(cdll, M, N, 512, epi=BIAS)[:2] == ("svla_nt_as_f0", AS)      # no sign bits: nothing to guard


def test_queries_refuse_bad_shapes(cdll):
    """shapes and activations the GEMM entries refuse; epilogue combinations and leading dimensions are the entries' own checks"""
    buf, out = ctypes.create_string_buffer(96), (ctypes.c_int * 12)()
    b, o = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(out, ctypes.c_void_p)
    for bad in (dict(M=0), dict(N=192), dict(K=48), dict(act=3), dict(n_cu=0)):
        a = dict(dict(M=256, N=512, K=512, act=0, out_f32=0, epi=0, alpha=1.0, drop=0, row_mult=1, n_cu=256), **bad)
        assert cdll.svla_gemm_nt_plan(*a.values(), b, 96, o) == -1, bad
    assert cdll.svla_gemm_tn_plan(0, 512, 512, 1, 0, 256, b, 96, o) == -1 and cdll.svla_gemm_tn_plan(64, 192, 512, 1, 0, 256, b, 96, o) == -1


def test_a_missing_assembly_kernel_falls_to_the_next_path(tmp_path):
    """gemm_host.h compiles with a plain host compiler; with the predicate false for a name the plan is what the next path of the chain gives:
    A-stationary -> output-stationary -> 8-phase; svla_tn_os -> gemm_tn8p"""
    from safevla_amd import build
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or os.path.join(os.path.dirname(build.CLANG), "clang++")
    exe = str(tmp_path / "gemm_plan_has")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "safevla_amd", "csrc"), os.path.join(ROOT, "tests", "helpers", "gemm_plan_has.cpp"),
                    "-o", exe], check=True)
    run = lambda missing: subprocess.run([exe, missing], check=True, capture_output=True, text=True).stdout.splitlines()
    f0, br, tn_os = "svla_nt_as_f0 0 741376 0 256x1 512 0 1 0 1", "svla_nt_os_br 1 741376 100 256x1 0 0 0 1024 1", "svla_tn_os 0 741376 11584 256 0 1"
    br_8p = "gemm_nt8p_bf16_kernel 2 741476 0 256x1 0 0 0 1024 1"
    assert run("-") == [f0, br, tn_os]
    assert run("svla_nt_as_f0") == ["svla_nt_os_b 1 741376 0 256x1 0 0 0 0 1", br, tn_os]      # 5792 tiles of a bias-only K = 512 problem: output-stationary next
    assert run("svla_nt_os_br") == [f0, br_8p, tn_os]
    assert run("svla_tn_os") == [f0, br, "gemm_tn8p_bf16_kernel 1 741376 11584 256 0 1"]
    assert run("*") == ["gemm_nt8p_bf16_kernel 2 741376 0 256x1 0 0 0 0 1", br_8p, "gemm_tn8p_bf16_kernel 1 741376 11584 256 0 1"]
