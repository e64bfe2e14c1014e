"""What svla_attn_fwd_bf16 / svla_attn_bwd_bf16 (include/svla.h) refuse, per kernel family behind them (csrc/attn_host.h: one AttnLimits row each).  A refused
call returns SVLA_EINVAL (-1) from host code before any HIP call, so every case below runs without a GPU and is harmless with one.  ONLY refused calls belong
here: an accepted call would go on to launch a kernel on the dummy pointers.  (What the families compute: tests/test_kernels_gpu.py, test_attn_hd96_gpu.py,
test_attn_long_bwd_gpu.py, test_attn_decode_long_gpu.py.)"""
import ctypes

import pytest

P = ctypes.c_void_p
FWD_ARGS = [("Q", P), ("K", P), ("V", P), ("ld", ctypes.c_long), ("O", P), ("ldo", ctypes.c_long), ("LSE", P),
            ("rows", ctypes.c_int), ("S", ctypes.c_int), ("H", ctypes.c_int), ("head_dim", ctypes.c_int), ("scale", ctypes.c_float), ("mask_mode", ctypes.c_int),
            ("traj", P), ("bias", P), ("kvalid", P), ("Sq", ctypes.c_int), ("ldq", ctypes.c_long), ("kv_rows", ctypes.c_int), ("drop", P), ("stream", P)]
BWD_ARGS = [("Q", P), ("K", P), ("V", P), ("ld", ctypes.c_long), ("O", P), ("ldo", ctypes.c_long), ("LSE", P), ("dO", P), ("lddo", ctypes.c_long),
            ("dQ", P), ("dK", P), ("dV", P), ("ldd", ctypes.c_long),
            ("rows", ctypes.c_int), ("S", ctypes.c_int), ("H", ctypes.c_int), ("head_dim", ctypes.c_int), ("scale", ctypes.c_float), ("mask_mode", ctypes.c_int),
            ("traj", P), ("bias", P), ("kvalid", P), ("Sq", ctypes.c_int), ("ldq", ctypes.c_long), ("lddq", ctypes.c_long), ("D_ws", P), ("drop", P), ("stream", P)]
PTR = 0x10000      # never dereferenced by a refused call; only has to be non-null
# a call every 64-wide family takes; 96-wide cases widen the strides below
BASE = dict(Q=PTR, K=PTR, V=PTR, ld=1536, O=PTR, ldo=512, LSE=PTR, dO=PTR, lddo=512, dQ=PTR, dK=PTR, dV=PTR, ldd=1536, rows=2, S=64, H=8, head_dim=64,
            scale=0.125, mask_mode=0, traj=None, bias=None, kvalid=None, Sq=0, ldq=0, lddq=0, kv_rows=0, D_ws=None, drop=None, stream=None)
HD96 = dict(head_dim=96, ld=2304, ldo=768, lddo=768, ldd=2304)
BLOCK_CAUSAL = 1


@pytest.fixture(scope="module")
def cdll():
    from safevla_amd import build
    lib = ctypes.CDLL(build.build())
    for name, args in (("svla_attn_fwd_bf16", FWD_ARGS), ("svla_attn_bwd_bf16", BWD_ARGS)):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = [t for _, t in args], ctypes.c_int
    return lib


def _call(cdll, which, **kw):
    a = dict(BASE, **kw)
    fn, args = (cdll.svla_attn_fwd_bf16, FWD_ARGS) if which == "fwd" else (cdll.svla_attn_bwd_bf16, BWD_ARGS)
    return fn(*[a[n] for n, _ in args])


FWD = [
    dict(S=0), dict(S=513), dict(ld=1537), dict(head_dim=80),                              # 64-wide tile / decode kernels
    dict(mask_mode=BLOCK_CAUSAL), dict(Sq=65), dict(kv_rows=10),
    dict(HD96, S=300), dict(HD96, bias=PTR), dict(HD96, mask_mode=2), dict(HD96, ldo=770),  # 96-wide
    dict(S=1025, Sq=1, ldq=512), dict(S=600, Sq=1, ldq=512, bias=PTR),                      # single-query decode above 512 keys
    dict(S=600, Sq=1, ldq=512, mask_mode=2), dict(S=600, Sq=1, ldq=516), dict(S=600, Sq=1, ldq=512, kv_rows=599),
    dict(S=600, Sq=2, ldq=512),                                                             # more than one query: no form above 512 keys
]
BWD_64 = [
    dict(rows=0), dict(H=0), dict(S=0), dict(S=513), dict(head_dim=80), dict(ld=1540), dict(lddo=516),
    dict(mask_mode=BLOCK_CAUSAL), dict(Sq=65), dict(Sq=1, ldq=516, lddq=512), dict(Sq=1, ldq=512, lddq=516),
]
BWD_LONG = [dict(c, S=300) for c in (
    dict(bias=PTR), dict(mask_mode=2), dict(mask_mode=BLOCK_CAUSAL), dict(ldo=516), dict(ldd=1538), dict(Sq=1, ldq=512, lddq=514))]
BWD_96 = [dict(HD96, **c) for c in (
    dict(S=257), dict(bias=PTR), dict(mask_mode=2), dict(ldo=772), dict(ldd=2306), dict(Sq=1, ldq=768, lddq=770))]


def _id(c):      # what the case changes in BASE (a 96-wide case: in the 96-wide base)
    wide = c.get("head_dim") == 96
    base = dict(BASE, **HD96) if wide else BASE
    return ("hd96," if wide else "") + ",".join(f"{k}={v}" for k, v in c.items() if base[k] != v)


@pytest.mark.parametrize("case", FWD, ids=_id)
def test_forward_refuses(cdll, case):
    assert _call(cdll, "fwd", **case) == -1


@pytest.mark.parametrize("case", BWD_64 + BWD_LONG + BWD_96, ids=_id)
def test_backward_refuses(cdll, case):
    assert _call(cdll, "bwd", **case) == -1

