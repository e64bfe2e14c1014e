"""svla_rows_gather and svla_fusion_text_bwd_seg (include/svla.h, csrc/rows.hip): both are exported with the header's argument order, and what they refuse is a host
check that returns SVLA_EINVAL (-1) before any launch -- so it holds on a machine without a GPU (the mechanism of tests/test_action_metrics_cabi_cpu.py; the GPU
side is in tests/test_rows_gather_gpu.py and tests/test_il_ragged_gpu.py)."""
import ctypes

import pytest

GATHER, SEG = "svla_rows_gather", "svla_fusion_text_bwd_seg"


@pytest.fixture(scope="module")
def lib():
    from safevla_amd import build
    from safevla_amd._lib import parse_header

    cdll = ctypes.CDLL(build.build())
    decls = parse_header()
    for name in (GATHER, SEG):
        fn = getattr(cdll, name)          # AttributeError: the symbol is missing
        fn.restype, fn.argtypes = ctypes.c_int, [ct for _, ct in decls[name]]
    return cdll, decls


def _call(lib, name, base, **over):
    cdll, decls = lib
    assert [n for n, _ in decls[name]] == list(base), decls[name]          # the argument order of the header
    base = dict(base)
    base.update(over)
    return getattr(cdll, name)(*base.values())


GATHER_BASE = dict(dst=4096, dst_stride=1024, src=8192, src_stride=1024, idx=64, rows=9, row_bytes=1024, src_rows=5, stream=None)
GATHER_REFUSED = [dict(rows=0), dict(rows=-2), dict(src_rows=0), dict(row_bytes=0), dict(row_bytes=1000), dict(row_bytes=1032, dst_stride=2048, src_stride=2048),
                  dict(dst_stride=1016), dict(src_stride=1016), dict(dst_stride=1008), dict(src_stride=512), dict(dst_stride=1032), dict(idx=None), dict(dst=None),
                  dict(src=None), dict(dst=4100), dict(src=8200)]


@pytest.mark.parametrize("over", GATHER_REFUSED)
def test_rows_gather_refusals(lib, over):
    assert _call(lib, GATHER, GATHER_BASE, **over) == -1


SEG_BASE = dict(dx0=64, seg=64, U=3, S=175, L=6, text_off=169, D=512, dtext=64, stream=None)
SEG_REFUSED = [dict(U=0), dict(L=0), dict(text_off=-1), dict(text_off=170), dict(D=0), dict(D=516), dict(dx0=None), dict(seg=None), dict(dtext=None)]


@pytest.mark.parametrize("over", SEG_REFUSED)
def test_fusion_text_bwd_seg_refusals(lib, over):
    assert _call(lib, SEG, SEG_BASE, **over) == -1


def test_new_entry_points_sit_in_front_of_the_last_one():
    """svla_replay_calls numbers the entry points in declaration order: the two new ones move only svla_attn_causal_fwd_bf16 (tests/test_attn_causal_long_cabi_cpu.py
    keeps it last)"""
    from safevla_amd._lib import parse_header

    assert list(parse_header())[-3:] == [GATHER, SEG, "svla_attn_causal_fwd_bf16"]
