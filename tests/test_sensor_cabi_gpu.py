"""C ABI of the reduced sensor sets (include/svla.h): ``svla_decoder_embed_fwd / _bwd`` and their fp32 twins with an absent term passed as NULL -- the in-hand pair,
the previous-action triple, or both -- against fp64 torch; a half-NULL group is refused and nothing is written; ``svla_acting_stage`` with a NULL in-hand pair
stages everything else as before."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
T, B, S = 3, 2, 5


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from safevla_amd import ops as o
    from safevla_amd.model import sensor_set      # noqa: F401  a tree without the sensor-subset contract would dereference the NULL tables on the device: fail here instead

    return o


def _inputs(D, dtype):
    g = torch.Generator().manual_seed(D)
    R = T * B
    d = dict(xf=torch.randn(R, S, D, generator=g).to(dtype), act=0.3 * torch.randn(22, D, generator=g), hand_t=0.3 * torch.randn(3, D, generator=g),
             div=torch.exp(torch.arange(0, D, 2) * (-math.log(10000.0) / D)), pa=torch.randint(0, 20, (T, B), generator=g),
             masks=torch.tensor([[0.0, 1.0], [1.0, 1.0], [1.0, 0.0]]), hand=torch.randint(0, 3, (T, B), generator=g), ts=torch.randint(0, 500, (T, B), generator=g),
             dout=(torch.randn(B * T, D, generator=g) / 128).to(dtype))      # six rows of |x| / 128 stay below the 0.25 up to which partials enter the shadow
    return {k: v.to(DEV) for k, v in d.items()}


@pytest.mark.parametrize("stride_rows", [1, S], ids=["ld=D", "ld=S*D"])
@pytest.mark.parametrize("with_act,with_hand", [(True, False), (False, True), (False, False)], ids=["no-hand", "no-action", "neither"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("D", [512, 768])
def test_decoder_embed_with_absent_terms_vs_fp64(ops, D, dtype, with_act, with_hand, stride_rows):
    d = _inputs(D, dtype)
    R = T * B
    xf = d["xf"] if stride_rows == S else d["xf"][:, 0].contiguous()          # position-0 rows inside [R, S, D], or packed [R, D] (a pruned last layer)
    out = torch.empty(B * T, D, device=DEV, dtype=dtype)
    ops.decoder_embed_fwd(xf, stride_rows * D, d["act"] if with_act else None, d["hand_t"] if with_hand else None, d["div"], d["pa"] if with_act else None,
                          d["masks"] if with_act else None, d["hand"] if with_hand else None, d["ts"], T, B, out)
    ang = d["ts"].double().unsqueeze(-1) * d["div"].double()
    pe = torch.zeros(T, B, D, dtype=torch.float64, device=DEV)
    pe[..., 0::2], pe[..., 1::2] = torch.sin(ang), torch.cos(ang)
    idx = torch.where(d["masks"] != 0, d["pa"], torch.full_like(d["pa"], 20))
    want = d["xf"][:, 0].double().view(T, B, D)
    if with_act:
        want = want + d["act"].double()[idx]
    if with_hand:
        want = want + d["hand_t"].double()[d["hand"]]
    want = pe + want
    got = out.double().view(B, T, D).permute(1, 0, 2)
    # fp32 sin / cos of arguments up to 500 (ulp(500) = 3e-5) and fp32 additions: 2e-4; bf16 adds one rounding of the sum: half an ulp <= 2^-8 relative
    tol = 2e-4 + (2.0 ** -8 * want.abs() if dtype == torch.bfloat16 else 0.0)
    assert ((got - want).abs() <= tol).all(), (got - want).abs().max().item()

    # ---- backward: the row copy into dxf at either stride, table gradients of the tables present only; with and without the deterministic shadow (bf16 kernel)
    d_tb = d["dout"].double().view(B, T, D).permute(1, 0, 2).reshape(R, D)
    for det in ((False, True) if dtype == torch.bfloat16 else (False,)):
        dxf = torch.full((R, stride_rows, D), 7.0, device=DEV, dtype=dtype)
        flat = torch.zeros(25 * D, device=DEV)
        da, dh = flat[:22 * D].view(22, D), flat[22 * D:].view(3, D)
        shadow = torch.zeros(25 * D, device=DEV, dtype=torch.int64)
        if det:
            ops.det_config(0, flat, shadow)
        try:
            ops.decoder_embed_bwd(d["dout"], d["pa"] if with_act else None, d["masks"] if with_act else None, d["hand"] if with_hand else None, T, B, dxf,
                                  stride_rows * D, da if with_act else None, dh if with_hand else None)
            if det:
                assert float(flat.abs().sum()) == 0.0          # everything went to the fixed-point shadow
                ops.det_finalize(flat, shadow)
        finally:
            if det:
                ops.det_config(0, None, None)
        assert torch.equal(dxf[:, 0].double(), d_tb) and (dxf[:, 1:] == 7).all()
        want_a = torch.zeros(22, D, dtype=torch.float64, device=DEV).index_add_(0, idx.reshape(R), d_tb)
        want_h = torch.zeros(3, D, dtype=torch.float64, device=DEV).index_add_(0, d["hand"].reshape(R), d_tb)
        # at most 6 rows meet in one table row: fp32 sums of values below 0.05 (ulp 4e-9 each); an absent table's gradient stays untouched
        assert (da.double() - (want_a if with_act else 0)).abs().max().item() < 1e-7, (det, "d act")
        assert (dh.double() - (want_h if with_hand else 0)).abs().max().item() < 1e-7, (det, "d hand")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_half_null_groups_are_refused_and_nothing_is_written(ops, dtype):
    from safevla_amd._lib import SvlaError

    D = 512
    d = _inputs(D, dtype)
    R = T * B
    full = dict(act=d["act"], hand_t=d["hand_t"], pa=d["pa"], masks=d["masks"], hand=d["hand"])
    for gone in (("hand",), ("hand_t",), ("act",), ("pa",), ("masks",), ("act", "pa"), ("pa", "masks")):
        a = {k: (None if k in gone else v) for k, v in full.items()}
        out = torch.full((B * T, D), 7.0, device=DEV, dtype=dtype)
        with pytest.raises(SvlaError, match="invalid argument"):
            ops.decoder_embed_fwd(d["xf"], S * D, a["act"], a["hand_t"], d["div"], a["pa"], a["masks"], a["hand"], d["ts"], T, B, out)
        dxf = torch.full((R, S, D), 7.0, device=DEV, dtype=dtype)
        da, dh = torch.full((22, D), 7.0, device=DEV), torch.full((3, D), 7.0, device=DEV)
        with pytest.raises(SvlaError, match="invalid argument"):
            ops.decoder_embed_bwd(d["dout"], a["pa"], a["masks"], a["hand"], T, B, dxf, S * D, None if a["act"] is None else da, None if a["hand_t"] is None else dh)
        torch.cuda.synchronize()
        assert (out == 7).all() and (dxf == 7).all() and (da == 7).all() and (dh == 7).all(), gone


def test_acting_stage_without_the_in_hand_pair(ops):
    from safevla_amd._lib import SvlaError

    g = torch.Generator(device=DEV).manual_seed(2)
    Bn, L, MS, t = 5, 7, 500, 37
    tok = torch.randn(Bn, 1, 84, 384, device=DEV, generator=g).to(torch.bfloat16)          # one camera
    pa = torch.randint(0, 20, (1, Bn), device=DEV, generator=g)
    mk = (torch.rand(1, Bn, 1, device=DEV, generator=g) > 0.2).float()
    ts = torch.randint(0, 600, (1, Bn), device=DEV, generator=g)
    ids = torch.randint(0, 5, (1, Bn, L), device=DEV, generator=g)
    z = lambda *s, dt=torch.int64: torch.zeros(*s, dtype=dt, device=DEV)
    d = dict(tok=torch.zeros_like(tok), pa=z(Bn), mk=z(Bn, dt=torch.float32), ts=z(Bn), ids=z(Bn, L), am=z(Bn, L), am8=z(Bn, L, dt=torch.uint8),
             kv=torch.full((Bn, MS), 7, dtype=torch.uint8, device=DEV), t_dev=z(()))
    seeds = [torch.tensor([v], dtype=torch.int32, device=DEV) for v in (5, 0x7FFFFFF0, -3)]
    want_seeds = [s_.clone().add_(0x3C6EF35) for s_ in seeds]
    ops.acting_stage(tok, d["tok"], pa, d["pa"], mk, d["mk"], None, None, ts, d["ts"], ids, d["ids"], d["am"], d["am8"], d["kv"], d["t_dev"], Bn, L, MS, t, seeds, 0x3C6EF35)
    torch.cuda.synchronize()
    assert torch.equal(d["tok"], tok) and torch.equal(d["pa"], pa.reshape(Bn)) and torch.equal(d["mk"], mk.reshape(Bn))
    assert torch.equal(d["ts"], ts.reshape(Bn)) and torch.equal(d["ids"], ids.reshape(Bn, L)) and int(d["t_dev"]) == t
    am = (ids.reshape(Bn, L) != 0).to(torch.int64); am[:, 0] = 1
    assert torch.equal(d["am"], am) and torch.equal(d["am8"], am.to(torch.uint8))
    ar = torch.arange(MS, device=DEV)
    assert torch.equal(d["kv"], ((ar[None, :] <= t) & (ar[None, :] >= torch.clamp(t - ts.reshape(Bn), min=0)[:, None])).to(torch.uint8))
    for a, b in zip(seeds, want_seeds):
        assert torch.equal(a, b)
    # one member of the pair alone: refused, nothing staged
    hand_dst = torch.full((Bn,), 7, dtype=torch.int64, device=DEV)
    d["kv"].fill_(7)
    with pytest.raises(SvlaError, match="invalid argument"):
        ops.acting_stage(tok, d["tok"], pa, d["pa"], mk, d["mk"], None, hand_dst, ts, d["ts"], ids, d["ids"], d["am"], d["am8"], d["kv"], d["t_dev"], Bn, L, MS, t + 1, seeds, 0x3C6EF35)
    torch.cuda.synchronize()
    assert (hand_dst == 7).all() and (d["kv"] == 7).all() and int(d["t_dev"]) == t
