"""What svla_attn_causal_fwd_bf16 (include/svla.h, csrc/attn_seq_long.hip) refuses: host checks that return SVLA_EINVAL (-1) before any launch, so they hold on a
machine without a GPU (the mechanism of tests/test_attn_decode_rows_cabi_cpu.py; the GPU side, with outputs that stay untouched, is in
tests/test_attn_causal_long_gpu.py).  Also: the entry is declared LAST in the header, so the ids svla_replay_calls gives the other entry points did not move."""
import ctypes

import pytest

NAME = "svla_attn_causal_fwd_bf16"


@pytest.fixture(scope="module")
def lib():
    from safevla_amd import build
    from safevla_amd._lib import parse_header

    cdll = ctypes.CDLL(build.build())
    decls = parse_header()
    fn = getattr(cdll, NAME)
    fn.restype, fn.argtypes = ctypes.c_int, [ct for _, ct in decls[NAME]]
    return cdll, decls


def _call(lib, **over):
    cdll, decls = lib
    base = dict(Q=64, K=64, V=64, ld=1536, O=64, ldo=512, LSE=None, rows=3, S=1000, H=8, head_dim=64, scale=0.125, traj=None, stream=None)
    assert [n for n, _ in decls[NAME]] == list(base), decls[NAME]          # the argument order of the header
    base.update(over)
    return getattr(cdll, NAME)(*base.values())


@pytest.mark.parametrize("over", [dict(head_dim=96), dict(head_dim=0), dict(rows=0), dict(rows=-2), dict(H=0), dict(H=-1), dict(S=0), dict(S=-1), dict(S=1025),
                                  dict(ld=1540), dict(ld=504), dict(ldo=516), dict(ldo=504), dict(Q=None), dict(K=None), dict(V=None), dict(O=None)])
def test_attn_causal_fwd_refusals(lib, over):
    assert _call(lib, **over) == -1


def test_the_entry_is_declared_last(lib):
    _, decls = lib
    assert list(decls)[-1] == NAME
