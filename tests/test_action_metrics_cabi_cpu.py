"""What svla_action_metrics_f32 (include/svla.h, csrc/metrics.hip) refuses: host checks that return SVLA_EINVAL (-1) before any launch, so they hold on a machine
without a GPU (the mechanism of tests/test_policy_sample_cabi_cpu.py; the GPU side is in tests/test_action_metrics_gpu.py).  pred = NULL is an allowed call, so it
is not among them: with it, every other refusal is still returned, and the check of the pointers does not name it."""
import ctypes

import pytest

NAME = "svla_action_metrics_f32"


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
    base = dict(logits=64, ld=23, target=64, rows=5, A=20, ignore_index=-1, counts=64, sums=64, pred=64, stream=None)
    assert [n for n, _ in decls[NAME]] == list(base), decls[NAME]          # the argument order of the header
    base.update(over)
    return getattr(cdll, NAME)(*base.values())


REFUSED = [dict(rows=0), dict(rows=-3), dict(A=0), dict(A=65), dict(ld=19), dict(logits=None), dict(target=None), dict(counts=None), dict(sums=None)]


@pytest.mark.parametrize("over", REFUSED)
def test_action_metrics_refusals(lib, over):
    assert _call(lib, **over) == -1
    assert _call(lib, pred=None, **over) == -1


def test_pred_null_is_not_among_the_refusals():
    """The entry's one check, read from the source: it names the four required pointers and not pred (a call with pred = NULL and valid arguments launches, which
    needs a GPU: tests/test_action_metrics_gpu.py::test_pred_none)."""
    import os
    import re

    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "safevla_amd", "csrc", "metrics.hip")).read()
    host = src[src.index('extern "C" int ' + NAME):]
    check = re.search(r"if \((.*?)\) return SVLA_EINVAL;", host, flags=re.S).group(1)
    assert all(f"!{p}" in check for p in ("logits", "target", "counts", "sums")) and "pred" not in check, check
    assert not any("pred" in over for over in REFUSED)
