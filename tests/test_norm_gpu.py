"""svla_norm_fwd_* / svla_norm_bwd_* (csrc/norm.hip) through ops.norm_fwd / ops.norm_bwd against ONE fp64 restatement on the CPU (``ref_norm`` below; gradients by
autograd), over every argument of the four entry points.  bf16 kernels get bf16-exact inputs, the fp32 twins the same values as float.

Tolerances (the ladder of test_kernels_gpu.py / test_fp32_mode_gpu.py::test_norm_f32_fwd_bwd):
    y                      bf16 8e-3 / 8e-3        fp32 max|err| / max|want| < 1e-5
    dx, dx_drop            bf16 1e-2 / 1e-2        fp32 the same < 1e-5
    dgamma, dbeta, dtok    bf16 rtol 2e-3, atol 2e-3 * max|want|        fp32 the same < 1e-4
    mean                   |err| <= 1e-6 |want| (forward matrix and statistics rows; on the zero-centred rows of the other cases 1e-6 * the row's mean |x|)
    rstd                   |err| <= 1e-5 |want|          (both kernels keep the statistics in fp32)
    y of the fp32 twin on the rows of ``stat_rows``: |err| <= 1e-4

What the three statistics gates rest on: the error of the restatement itself, measured on the CPU by running ``ref_norm`` in fp32 against ``ref_norm`` in fp64
on the eight offset rows of ``stat_rows`` (offset 1024 / std 16 and offset 256 / std 4, seed 40, LayerNorm, gamma = 1), next to a one-pass fp32 form
(variance = E[x^2] - mean^2):
                          two-pass fp32                                one-pass fp32
    D = 512    rstd 1.5e-7   mean 0 (sums exact)   y 3.8e-7          rstd 2.1e-4   y 5.3e-4
    D = 768    rstd 1.9e-7   mean 4.0e-8           y 2.8e-6          rstd 3.3e-4   y 1.1e-3
(rstd, mean: relative; y: absolute; RMSNorm two-pass: rstd 5.4e-8 / 1.2e-7, y 9.2e-8 / 1.3e-7.)  So the rstd gate of 1e-5 leaves the two-pass form 50x of room,
the hardware rsqrt included, and sits 20x under the one-pass form; the y gate of 1e-4 separates the two by 5x and more.  bf16 y cannot separate them (its rounding
is 4e-3), which is why the statistics and the fp32 twin carry this check.  One row sits close to the y gate by construction: 1000 with a single 1008 at D = 768 has
the mean 1000 + 8 / 768, which fp32 holds to 2.0e-5; times rstd 3.47 that is 7.1e-5 in every y of the row (measured 7.6e-5 with torch's fp32 mean, 7.1e-5 with the
kernel's sum * (1 / D)), times gamma -- so the statistics cases draw gamma within a few percent of 1, as the gate assumes.  The kernels on an MI355X, same rows:
rstd within 1.0e-7, mean within 4.0e-8, fp32 y within 5.2e-7 (D = 512) and 7.4e-5 (D = 768: the 1000 / 1008 row).

ReLU boundary: an element whose fp64 pre-activation is within 1e-5 of zero may fall on either side in fp32.  A row with such an element gets dy = 0 in the kernel's
input and in the reference alike (so it adds nothing to dgamma / dbeta / dtok on either side) and is left out of the dx comparison; at most 2 % of a case's rows
may go that way (asserted where the case is built; the seeds are chosen so that the reference alone stays within it).  Rows left out, per case with ReLU:
    rows 1, 2, 7, 9: none in any case
    backward matrix / accumulate / without-dgamma cases at 333 rows: D = 512 LayerNorm 0, RMSNorm 2 (0.6 %); D = 768 LayerNorm 1 (0.3 %), RMSNorm 3 (0.9 %)
    row maps at 333 rows: 1 (0.3 %) at D = 384 LayerNorm, 768 both norms, 1024 both norms; 0 elsewhere
    grid-stride forward 62 of 16 393 (0.38 %), backward 143 of 32 779 (0.44 %)"""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_gemm_ld_gpu import SENT_BF16, SENT_F32, _bits
from test_kernels_gpu import DEV, _keep_np, bf, close, ops, rnd      # noqa: F401  (ops: fixture)

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp32": torch.float32}
ID = (0, 0, 0)
SPARE = 3                                     # rows behind the last group of a mapped buffer
TOK_MAPS = {84: (84, 97, 5), 168: (168, 181, 1)}      # one camera group / the product's two (model.py: ymap = (ncam * 84, S, 1))
RELU_EDGE = 1e-5
DROP_SEED, DROP_STREAM, DROP_P = 5, 1, 0.1


# ------------------------------------------------------------------------------------------------ reference
def ref_norm(x, gamma, beta, eps, rms, relu=False, tok=None, G=0, tok_group=0):
    """The logical op on [rows, D] in the dtype of ``x``: z = norm(x) * gamma (+ beta) -> optional ReLU -> optional + tok[(m % G) / tok_group].
    Returns (z, pre-activation, mean, rstd).  Two passes: the mean, then the mean of the squared deviations."""
    if rms:
        mean = torch.zeros(x.shape[0], dtype=x.dtype)
        xc = x
    else:
        mean = x.mean(-1)
        xc = x - mean[:, None]
    rstd = torch.rsqrt(xc.pow(2).mean(-1) + eps)
    pre = xc * rstd[:, None] * gamma
    if beta is not None and not rms:
        pre = pre + beta
    z = torch.relu(pre) if relu else pre
    if tok is not None:
        m = torch.arange(x.shape[0])
        z = z + tok[((m % G) if G > 0 else m) // tok_group]
    return z, pre, mean, rstd


def map_rows(rows, mp):
    """memory row of every logical row: (m // G) * GS + OFF + m % G"""
    G, GS, OFF = mp
    m = torch.arange(rows)
    return m if G == 0 else (m // G) * GS + OFF + m % G


def buf_rows(rows, mp):
    G, GS, _ = mp
    return rows if G == 0 else ((rows - 1) // G + 1) * GS + SPARE


def stat_rows(D, rms, seed):
    """(x, dy) of the rows a wrong variance formula gets wrong: 4 rows at offset 1024 / std 16, 4 at offset 256 / std 4, a constant row of 300, a row of 1000 with
    a single 1008, an all-zero row.  dy of each row is scaled by the power of two next to 1 / rstd, so that every dx row is O(1) and the dx gate means the same
    on each."""
    x = torch.cat([bf(1024 + 16 * rnd(4, D, seed=seed)), bf(256 + 4 * rnd(4, D, seed=seed + 1)), torch.full((1, D), 300.0), torch.full((1, D), 1000.0),
                   torch.zeros(1, D)])
    x[9, 5] = 1008.0
    assert torch.equal(bf(x), x)
    rstd = ref_norm(x.double(), torch.ones(D, dtype=torch.float64), None, 1e-5, rms)[3]
    dy = bf(rnd(x.shape[0], D, seed=seed + 2) * torch.exp2(torch.round(-torch.log2(rstd))).float()[:, None])
    return x, dy


STAT_OFFSET_ROWS = slice(0, 8)                # the rows behind the measurement of the module docstring


@functools.lru_cache(maxsize=None)
def make_case(D, rms, rows, eps=1e-5, relu=False, tok=None, dres=False, kind="std", seed=11):
    """Inputs (CPU, float) and the fp64 reference of one logical problem; shared by every test that asks for the same one and never modified.
    ``tok`` = (G, tok_group): the token add of the forward / dtok of the backward; ``kind``: std = N(0.3, 2) rows, pos = N(3, 1.5) rows (every row mean well away
    from zero: the mean gate is relative), stats = stat_rows."""
    if kind == "stats":
        x, dy = stat_rows(D, rms, seed)
        assert rows == x.shape[0]
    else:
        x = bf(rnd(rows, D, seed=seed) * 1.5 + 3) if kind == "pos" else bf(rnd(rows, D, seed=seed) * 2 + 0.3)
        dy = bf(rnd(rows, D, seed=seed + 1))
    c = SimpleNamespace(D=D, rms=rms, rows=rows, eps=eps, relu=relu, tok_cfg=tok, use_dres=dres, x=x)
    # stats: gamma within a few percent of 1, because the absolute y gate of the fp32 twin is stated for gamma ~ 1 (module docstring: the 1000 / 1008 row)
    c.gamma, c.beta, c.tok = 1 + (0.01 if kind == "stats" else 0.1) * rnd(D, seed=seed + 3), 0.1 * rnd(D, seed=seed + 4), rnd(2, D, seed=seed + 5)
    c.dres = bf(rnd(rows, D, seed=seed + 2))
    c.start = rnd(4, D, seed=seed + 6)          # non-zero starting values of dgamma, dbeta, dtok[0], dtok[1]
    G, tok_group = tok if tok else (0, 0)
    xx, gg, bb, tt = [t.double().requires_grad_(True) for t in (x, c.gamma, c.beta, c.tok)]
    z, pre, mean, rstd = ref_norm(xx, gg, bb, float(np.float32(eps)), rms, relu, tt if tok else None, G, tok_group)
    c.edge = (pre.detach().abs() < RELU_EDGE).any(-1) if relu else torch.zeros(rows, dtype=torch.bool)
    c.edge_share = c.edge.float().mean().item()
    assert c.edge_share <= 0.02, f"{int(c.edge.sum())} of {rows} rows have a pre-activation within {RELU_EDGE} of zero: more than 2 % left out"
    c.dy = dy.clone()
    c.dy[c.edge] = 0
    z.backward(c.dy.double())
    c.z, c.mean, c.rstd = z.detach(), mean.detach(), rstd.detach()
    # what the mean's error is relative to: the mean itself on pos / stats rows (the stated gate); on std rows, whose mean of 0.3 +- 0.09 can come out next to
    # zero, the row's mean |x| -- the rounding error of a sum scales with the sum of the magnitudes, and on rows of one sign the two are the same thing
    c.mean_scale = x.abs().double().mean(-1) if kind == "std" else None
    c.dx = xx.grad + (c.dres.double() if dres else 0)
    c.dgamma, c.dbeta, c.dtok = gg.grad, (None if rms else bb.grad), (tt.grad if tok else None)
    return c


# ------------------------------------------------------------------------------------------------ buffers and gates
def place_in(t, mp, dtype):
    """logical [rows, D] -> device buffer in which the mapped rows hold ``t`` and every other row NaN"""
    if mp[0] == 0:
        return t.to(DEV).to(dtype)
    buf = torch.full((buf_rows(t.shape[0], mp), t.shape[1]), float("nan"), device=DEV, dtype=dtype)
    buf[map_rows(t.shape[0], mp).to(DEV)] = t.to(DEV).to(dtype)
    return buf


def sentinel_out(rows, mp, D, dtype):
    buf = torch.empty(buf_rows(rows, mp), D, device=DEV, dtype=dtype)
    _bits(buf).fill_(SENT_BF16 if dtype == torch.bfloat16 else SENT_F32)
    return buf


def take_out(buf, rows, mp, name):
    """the mapped rows of an output buffer, after checking that every other row still holds the sentinel bit for bit"""
    idx = map_rows(rows, mp).to(DEV)
    other = torch.ones(buf.shape[0], dtype=torch.bool, device=DEV)
    other[idx] = False
    assert (_bits(buf)[other] == (SENT_BF16 if buf.dtype == torch.bfloat16 else SENT_F32)).all(), f"{name}: rows outside the map were written"
    return buf[idx]


def same_bits(a, b, name):
    ne = _bits(a.contiguous()) != _bits(b.contiguous())
    assert not ne.any(), f"{name}: {int(ne.sum())} of {ne.numel()} elements differ, first at {tuple(ne.nonzero()[0].tolist())}"


GATES = {"y": ((8e-3, 8e-3), 1e-5), "dx": ((1e-2, 1e-2), 1e-5), "grad": ((2e-3, None), 1e-4)}


def check(got, want, what, dt, name):
    got, want = got.detach().double().cpu(), want.double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert torch.isfinite(got).all(), f"{name}: not finite"
    if got.numel() == 0:
        return
    (rtol, atol), rel_gate = GATES[what]
    if dt == "fp32":
        err = (got - want).abs().max().item() / (want.abs().max().item() + 1e-30)
        print(f"[{name} fp32] rel-to-max err {err:.3g} (gate {rel_gate:g})")
        assert err < rel_gate, f"{name}: max|err| / max|want| = {err:.3g} >= {rel_gate:g}"
    else:
        close(got, want, rtol, atol if atol is not None else rtol * want.abs().max().item(), name)


def check_stat(got, want, gate, name, scale=None):
    """|got - want| <= gate * |want| per row (``scale`` given: gate * scale)"""
    got, want = got.double().cpu(), want.double()
    scale = want.abs() if scale is None else scale.double()
    assert torch.isfinite(got).all(), f"{name}: not finite"
    err = (got - want).abs()
    rel = (err / scale.clamp_min(1e-300)).max().item() if (scale != 0).any() else 0.0
    print(f"[{name}] max rel err {rel:.3g} (gate {gate:g})")
    bad = err > gate * scale
    assert not bad.any(), f"{name}: row {int(bad.nonzero()[0])}: got {got[bad][0]:.9g} want {want[bad][0]:.9g} (relative gate {gate:g})"


# ------------------------------------------------------------------------------------------------ launches
def forward(ops, c, dt, xmap=ID, ymap=None, save_stats=True, name=""):
    """the forward of case ``c``: y (logical rows), mean, rstd, each checked against the reference"""
    tdt = DT[dt]
    G, tok_group = c.tok_cfg if c.tok_cfg else (0, 0)
    ymap = ymap if ymap is not None else (TOK_MAPS[G] if G else ID)
    assert not c.tok_cfg or ymap[0] == G
    yb = sentinel_out(c.rows, ymap, c.D, tdt)
    _, mean, rstd = ops.norm_fwd(place_in(c.x, xmap, tdt), c.gamma.to(DEV), None if c.rms else c.beta.to(DEV), c.eps, c.rows, D=c.D, rms=c.rms, relu=c.relu,
                                 tok=c.tok.to(DEV) if c.tok_cfg else None, tok_group=tok_group, y=yb, xmap=xmap, ymap=ymap, save_stats=save_stats)
    y = take_out(yb, c.rows, ymap, name + " y")
    check(y, c.z, "y", dt, name + " y")
    if save_stats:
        assert (mean is None) == c.rms
        if not c.rms:
            check_stat(mean, c.mean, 1e-6, name + " mean", scale=c.mean_scale)
        check_stat(rstd, c.rstd, 1e-5, name + " rstd")
    else:
        assert mean is None and rstd is None
    return y, mean, rstd


def backward(ops, c, dt, mean, rstd, dymap=None, xmap=ID, dxmap=ID, prefill=False, want_dgamma=True, want_dbeta=True, row_mult=None, name=""):
    """the backward of case ``c`` from the kernel's own saved statistics: dx (logical rows), dgamma, dbeta, dtok, dx_drop, each checked against the reference"""
    tdt = DT[dt]
    G, tok_group = c.tok_cfg if c.tok_cfg else (0, 0)
    dymap = dymap if dymap is not None else (TOK_MAPS[G] if G else ID)
    assert not c.tok_cfg or dymap[0] == G
    start = c.start if prefill else torch.zeros_like(c.start)
    dg = start[0].to(DEV) if want_dgamma else None
    db = start[1].to(DEV) if (want_dbeta and not c.rms) else None
    dtk = start[2:4].contiguous().to(DEV) if c.tok_cfg else None
    dxb = sentinel_out(c.rows, dxmap, c.D, tdt)
    dxd = sentinel_out(c.rows, ID, c.D, tdt) if row_mult else None
    drop = ops.Dropout(seed=DROP_SEED, stream=DROP_STREAM, p=DROP_P, row_mult=row_mult) if row_mult else None
    ops.norm_bwd(place_in(c.dy, dymap, tdt), place_in(c.x, xmap, tdt), c.gamma.to(DEV), None if c.rms else c.beta.to(DEV), mean, rstd, c.rows, dg, db, D=c.D,
                 rms=c.rms, relu=c.relu, dtok=dtk, tok_group=tok_group, dx=dxb, dymap=dymap, xmap=xmap, dxmap=dxmap,
                 dres=c.dres.to(DEV).to(tdt) if c.use_dres else None, dx_drop=dxd, drop=drop)
    dx = take_out(dxb, c.rows, dxmap, name + " dx")
    ok = ~c.edge
    check(dx[ok.to(DEV)], c.dx[ok], "dx", dt, name + " dx")
    if want_dgamma:
        check(dg, start[0].double() + c.dgamma, "grad", dt, name + " dgamma")
    if db is not None:
        check(db, start[1].double() + c.dbeta, "grad", dt, name + " dbeta")
    if dtk is not None:
        check(dtk, start[2:4].double() + c.dtok, "grad", dt, name + " dtok")
    if row_mult:
        idx = (np.arange(c.rows, dtype=np.uint64)[:, None] * np.uint64(row_mult * c.D)) + np.arange(c.D, dtype=np.uint64)[None, :]
        keep = _keep_np(DROP_SEED, DROP_STREAM, DROP_P, idx)
        assert 0.85 < keep.float().mean().item() < 0.95 or c.rows < 3
        got = dxd.float().cpu()
        assert (got[~keep] == 0).all(), f"{name} dx_drop: a dropped element is not exactly zero"
        want = c.dx * keep / (1.0 - float(np.float32(DROP_P)))
        sel = keep & ok[:, None]
        check(got[sel], want[sel], "dx", dt, name + " dx_drop kept elements")
    return SimpleNamespace(dx=dx, dgamma=dg, dbeta=db, dtok=dtk, dx_drop=dxd)


def norm_name(rms):
    return "rms" if rms else "ln"


# ------------------------------------------------------------------------------------------------ a. forward matrix
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("rms", [False, True], ids=norm_name)
@pytest.mark.parametrize("D", [384, 512, 768, 1024])
def test_forward_matrix(ops, D, rms, dt):
    """every forward width x norm x type at eps 1e-5 / 1e-6 and rows 1 (one wave, one row), 2 (a full pair), 7 and 9 (odd tails inside and across a workgroup of
    4 waves x 2 rows), statistics saved and not"""
    for eps in (1e-5, 1e-6):
        for rows in (1, 2, 7, 9):
            c = make_case(D, rms, rows, eps=eps, kind="pos", seed=100 + rows)
            name = f"fwd D={D} {norm_name(rms)} {dt} eps={eps:g} rows={rows}"
            y, _, _ = forward(ops, c, dt, name=name)
            y0, _, _ = forward(ops, c, dt, save_stats=False, name=name + " no stats")
            same_bits(y, y0, name + ": y with and without saved statistics")


# ------------------------------------------------------------------------------------------------ b. statistics
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("rms", [False, True], ids=norm_name)
@pytest.mark.parametrize("D", [512, 768])
def test_statistics_of_offset_constant_and_zero_rows(ops, D, rms, dt):
    """rows whose mean dwarfs their spread (see the module docstring), forward and backward: a variance taken as E[x^2] - mean^2 fails the rstd gate here"""
    c = make_case(D, rms, 11, kind="stats", seed=40)
    name = f"stats D={D} {norm_name(rms)} {dt}"
    y, mean, rstd = forward(ops, c, dt, name=name)
    eps32 = float(np.float32(c.eps))
    if rms:                                    # the all-zero row: y = 0, rstd = eps^-1/2
        assert (y[10] == 0).all() and abs(rstd[10].item() * eps32 ** 0.5 - 1) <= 1e-5
    else:                                      # the constant and the all-zero row: y = beta
        for r in (8, 10):
            check(y[r], c.beta, "y", dt, f"{name} row {r} = beta")
            assert abs(rstd[r].item() * eps32 ** 0.5 - 1) <= 1e-5
    if dt == "fp32":
        err = (y.double().cpu() - c.z).abs().max().item()
        print(f"[{name}] max |y err| {err:.3g} (gate 1e-4)")
        assert err <= 1e-4, f"{name}: |y err| {err:.3g} > 1e-4"
    backward(ops, c, dt, mean, rstd, name=name)


# ------------------------------------------------------------------------------------------------ c. grid-stride loop
needs_default_grid = pytest.mark.skipif("SVLA_NORM_GRID" in os.environ, reason="SVLA_NORM_GRID overrides the grid caps these row counts are chosen against")


@needs_default_grid
def test_forward_grid_stride(ops):
    """2048 * 8 + 9 rows: the first row count above norm_grid's forward cap, so some waves take a second trip through the row loop"""
    c = make_case(512, False, 2048 * 8 + 9, relu=True, seed=60)
    forward(ops, c, "bf16", name="fwd grid-stride")


@needs_default_grid
def test_backward_grid_stride(ops):
    """4096 * 8 + 11 rows: the first row count above the backward cap; dgamma / dbeta sum over every trip"""
    c = make_case(512, False, 4096 * 8 + 11, relu=True, seed=61)
    _, mean, rstd = forward(ops, c, "bf16", name="bwd grid-stride: fwd")
    backward(ops, c, "bf16", mean, rstd, name="bwd grid-stride")


# ------------------------------------------------------------------------------------------------ d. backward matrix
BWD_ROWS = (1, 2, 7, 9, 333)
VARIANTS = {
    "plain": dict(),
    "dres": dict(dres=True),                                        # RMSNorm + dres: the llama block's two norm backwards
    "relu": dict(relu=True),                                        # ReLU without a token add
    "relu_dres": dict(relu=True, dres=True),
    "tok_one_group": dict(relu=True, tok=(84, 84)),
    "tok_two_groups": dict(relu=True, tok=(168, 84)),
    "tok_identity_map": dict(relu=True, tok=(0, None)),             # tok_group = ceil(rows / 2): rows <= 2 * tok_group
    "tok_without_relu": dict(tok=(168, 84)),
    "tok_one_group_without_relu": dict(tok=(84, 84)),
}


def bwd_case(D, rms, rows, relu=False, tok=None, dres=False):
    if tok and tok[1] is None:
        tok = (0, (rows + 1) // 2)
    return make_case(D, rms, rows, relu=relu, tok=tok, dres=dres, seed=200 + rows)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("rms", [False, True], ids=norm_name)
@pytest.mark.parametrize("D", [512, 768])
def test_backward_matrix(ops, D, rms, dt, variant):
    for rows in BWD_ROWS:
        c = bwd_case(D, rms, rows, **VARIANTS[variant])
        name = f"bwd D={D} {norm_name(rms)} {dt} {variant} rows={rows}"
        _, mean, rstd = forward(ops, c, dt, name=name + ": fwd")
        backward(ops, c, dt, mean, rstd, name=name)


@pytest.mark.parametrize("variant", ["dres", "tok_two_groups", "tok_one_group", "tok_identity_map"])
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("rms", [False, True], ids=norm_name)
@pytest.mark.parametrize("D", [512, 768])
def test_backward_gradients_accumulate(ops, D, rms, dt, variant):
    """dgamma / dbeta / dtok start from non-zero values: result = start + sum (a one-group dtok leaves its second row at the start value)"""
    for rows in BWD_ROWS:
        c = bwd_case(D, rms, rows, **VARIANTS[variant])
        name = f"bwd prefilled D={D} {norm_name(rms)} {dt} {variant} rows={rows}"
        _, mean, rstd = forward(ops, c, dt, name=name + ": fwd")
        out = backward(ops, c, dt, mean, rstd, prefill=True, name=name)
        if c.tok_cfg and (c.tok_cfg == (84, 84) or rows == 1):
            assert torch.equal(out.dtok[1].cpu(), c.start[3]), f"{name}: dtok[1] has no rows and must keep its starting value"


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("rms", [False, True], ids=norm_name)
@pytest.mark.parametrize("D", [512, 768])
def test_backward_without_dgamma_or_dbeta(ops, D, rms, dt):
    """dgamma = NULL and / or dbeta = NULL: dx keeps its bits, the gradient that is still asked for its value; RMSNorm never touches dbeta"""
    for rows in BWD_ROWS:
        c = bwd_case(D, rms, rows, relu=True, tok=(168, 84))
        name = f"bwd D={D} {norm_name(rms)} {dt} rows={rows}"
        _, mean, rstd = forward(ops, c, dt, name=name + ": fwd")
        full = backward(ops, c, dt, mean, rstd, prefill=True, name=name)
        for wg, wb in ((False, True), (True, False), (False, False)):
            part = backward(ops, c, dt, mean, rstd, prefill=True, want_dgamma=wg, want_dbeta=wb, name=f"{name} dgamma={wg} dbeta={wb}")
            same_bits(part.dx, full.dx, f"{name} dgamma={wg} dbeta={wb}: dx")
    if rms:                                    # beta / dbeta given to an RMSNorm: ignored, dbeta keeps its bits
        c = bwd_case(D, True, 9)
        tdt = DT[dt]
        y, _, rstd = ops.norm_fwd(c.x.to(DEV).to(tdt), c.gamma.to(DEV), c.beta.to(DEV), c.eps, 9, D=D, rms=True)
        check(y, c.z, "y", dt, "rms with beta: y")
        dg, db = torch.zeros(D, device=DEV), c.start[1].to(DEV)
        dx = ops.norm_bwd(c.dy.to(DEV).to(tdt), c.x.to(DEV).to(tdt), c.gamma.to(DEV), c.beta.to(DEV), None, rstd, 9, dg, db, D=D, rms=True)
        check(dx, c.dx, "dx", dt, "rms with beta: dx")
        assert torch.equal(db.cpu(), c.start[1])


@pytest.mark.parametrize("row_mult", [1, 181])
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("rms", [False, True], ids=norm_name)
@pytest.mark.parametrize("D", [512, 768])
def test_backward_dropout_output(ops, D, rms, dt, row_mult):
    """dx_drop = dx * keep / (1 - p), keep = oracle.ref_model.hash_keep at element m * row_mult * D + col (8 values per lane at D = 512: two keep-groups of four,
    12 at D = 768: three): dropped elements exactly zero, kept ones against the fp64 dx -- never against the kernel's own"""
    for rows in BWD_ROWS:
        c = bwd_case(D, rms, rows)
        name = f"bwd D={D} {norm_name(rms)} {dt} row_mult={row_mult} rows={rows}"
        _, mean, rstd = forward(ops, c, dt, name=name + ": fwd")
        backward(ops, c, dt, mean, rstd, row_mult=row_mult, name=name)


# ------------------------------------------------------------------------------------------------ e. row maps
XMAP, YMAP, DXMAP = (5, 9, 2), (7, 12, 3), (3, 11, 4)      # three different (G, GS, OFF), each with GS > G + OFF


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("rms", [False, True], ids=norm_name)
@pytest.mark.parametrize("D", [384, 512, 768, 1024])
def test_row_maps_on_every_operand(ops, D, rms, dt):
    """xmap / ymap in the forward, dymap / xmap / dxmap in the backward: rows outside a map hold NaN (inputs) or a sentinel (outputs); no NaN reaches an output, no
    sentinel is touched, and y / dx equal the contiguous call on the gathered rows bit for bit (the atomically accumulated gradients: both at tolerance)"""
    for rows in (9, 333):
        c = make_case(D, rms, rows, relu=True, dres=True, seed=310 + rows)
        name = f"maps D={D} {norm_name(rms)} {dt} rows={rows}"
        y0, mean0, rstd0 = forward(ops, c, dt, name=name + " contiguous")
        y1, mean1, rstd1 = forward(ops, c, dt, xmap=XMAP, ymap=YMAP, name=name + " mapped")
        same_bits(y1, y0, name + " y")
        same_bits(rstd1, rstd0, name + " rstd")
        if not rms:
            same_bits(mean1, mean0, name + " mean")
        if D in (512, 768):
            b0 = backward(ops, c, dt, mean0, rstd0, prefill=True, name=name + " contiguous")
            b1 = backward(ops, c, dt, mean0, rstd0, dymap=YMAP, xmap=XMAP, dxmap=DXMAP, prefill=True, name=name + " mapped")
            same_bits(b1.dx, b0.dx, name + " dx")
