"""What svla_attn_decode_rows_bf16 / svla_kv_append_rows_bf16 (include/svla.h, csrc/attn_decode.hip) refuse: host checks that return SVLA_EINVAL (-1) before any
launch, so they hold on a machine without a GPU (the mechanism of tests/test_attn_cabi_cpu.py; the GPU side, with outputs that stay untouched, is in
tests/test_attn_decode_rows_gpu.py)."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from safevla_amd import build
    from safevla_amd._lib import parse_header

    cdll = ctypes.CDLL(build.build())
    decls = parse_header()
    for name in ("svla_attn_decode_rows_bf16", "svla_kv_append_rows_bf16"):
        fn = getattr(cdll, name)
        fn.restype, fn.argtypes = ctypes.c_int, [ct for _, ct in decls[name]]
    return cdll, decls


def _call(lib, name, **over):
    cdll, decls = lib
    base = {"svla_attn_decode_rows_bf16": dict(Q=64, ldq=1536, K=64, V=64, ld=1024, O=64, ldo=512, LSE=None, klen=64, cache_row=None, rows=5, H=8, head_dim=64, scale=0.125,
                                               kv_rows=1000, stream=None),
            "svla_kv_append_rows_bf16": dict(src=64, ld_src=1536, cache=64, cache_rows=1000, width=1024, cache_row=None, pos=64, rows=5, stream=None)}[name]
    assert [n for n, _ in decls[name]] == list(base), decls[name]          # the argument order of the header
    base.update(over)
    return getattr(cdll, name)(*base.values())


@pytest.mark.parametrize("over", [dict(rows=0), dict(rows=-2), dict(H=0), dict(head_dim=96), dict(head_dim=0), dict(kv_rows=0), dict(kv_rows=1025), dict(ld=1028),
                                  dict(ldq=1540), dict(ldo=516), dict(klen=None)])
def test_attn_decode_rows_refusals(lib, over):
    assert _call(lib, "svla_attn_decode_rows_bf16", **over) == -1


@pytest.mark.parametrize("over", [dict(rows=0), dict(width=0), dict(width=1020), dict(ld_src=1540), dict(cache_rows=0), dict(pos=None)])
def test_kv_append_rows_refusals(lib, over):
    assert _call(lib, "svla_kv_append_rows_bf16", **over) == -1
