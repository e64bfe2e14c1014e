"""What svla_norm_fwd_* / svla_norm_bwd_* (include/svla.h; host code at the end of csrc/norm.hip) refuse, for the bf16 entry points and their fp32 twins.  A
refused call returns SVLA_EINVAL (-1) from host code before any HIP call, so every case below runs without a GPU and is harmless with one.  ONLY refused calls
belong here: an accepted call would go on to launch a kernel on the dummy pointers.  (What the kernels compute: tests/test_norm_gpu.py.)"""
import ctypes

import pytest

PTR = 0x10000      # never dereferenced by a refused call; only has to be non-null
# calls that are accepted as they stand: every case changes what its id names
FWD_BASE = dict(x=PTR, xG=0, xGS=0, xOFF=0, gamma=PTR, beta=PTR, eps=1e-5, rows=4, D=512, rms=0, relu=0, tok=None, tok_group=0, y=PTR, yG=0, yGS=0, yOFF=0,
                mean=PTR, rstd=PTR, stream=None)
BWD_BASE = dict(dy=PTR, dyG=0, dyGS=0, dyOFF=0, x=PTR, xG=0, xGS=0, xOFF=0, gamma=PTR, beta=PTR, mean=PTR, rstd=PTR, rows=4, D=512, rms=0, relu=0, tok_group=0,
                dres=None, dx=PTR, dxG=0, dxGS=0, dxOFF=0, dgamma=PTR, dbeta=PTR, dtok=None, dx_drop=None, drop=None, stream=None)
KINDS = ("bf16", "f32")


@pytest.fixture(scope="module")
def entry():
    from safevla_amd import build
    from safevla_amd._lib import parse_header
    lib, decls = ctypes.CDLL(build.build()), parse_header()

    def call(name, base, case):
        fn, args = getattr(lib, name), decls[name]
        assert [n for n, _ in args] == list(base), name      # the header's argument names, in its order
        fn.argtypes, fn.restype = [t for _, t in args], ctypes.c_int
        a = dict(base, **case)
        return fn(*[a[n] for n, _ in args])
    return call


FWD = [
    dict(rows=0), dict(rows=-3), dict(D=256), dict(D=640),                                      # no rows; widths that are not built
    dict(tok=PTR, tok_group=0), dict(tok=PTR, tok_group=-1),                                    # a token add needs a group size
    dict(x=None), dict(gamma=None), dict(y=None),
    dict(xG=-1, xGS=8, xOFF=1), dict(yG=-5, yGS=8, yOFF=1),                                     # a row map's G is 0 (identity) or a group size
]
BWD = [
    dict(rows=0), dict(rows=-1), dict(D=384), dict(D=1024), dict(D=256),                        # forward-only widths are refused by the backward
    dict(dtok=PTR, tok_group=0), dict(dtok=PTR, tok_group=-1),
    dict(dy=None), dict(x=None), dict(gamma=None), dict(rstd=None), dict(dx=None),
    dict(mean=None),                                                                            # LayerNorm (rms = 0) reads mean[m]
    dict(dyG=-1, dyGS=8, dyOFF=1), dict(xG=-1, xGS=8, xOFF=1), dict(dxG=-2, dxGS=8, dxOFF=1),
    # dtok is [2, D]: more than two token groups (G_eff > 2 * tok_group, G_eff = dyG > 0 ? dyG : rows)
    dict(dtok=PTR, tok_group=84, dyG=252, dyGS=300, dyOFF=1),                                   # three camera groups
    dict(dtok=PTR, tok_group=84, dyG=169, dyGS=181, dyOFF=1),                                   # one row into a third group
    dict(dtok=PTR, tok_group=2, rows=5),                                                        # identity map: G_eff = rows
    dict(dtok=PTR, tok_group=1, rows=3),
    dict(dtok=PTR, tok_group=84, rms=1, mean=None, dyG=252, dyGS=300, dyOFF=1),                 # RMSNorm takes the same limit
]


def _id(c):
    return ",".join(f"{k}={v}" for k, v in c.items())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", FWD, ids=_id)
def test_forward_refuses(entry, case, kind):
    assert entry(f"svla_norm_fwd_{kind}", FWD_BASE, case) == -1


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", BWD, ids=_id)
def test_backward_refuses(entry, case, kind):
    assert entry(f"svla_norm_bwd_{kind}", BWD_BASE, case) == -1
