"""The streaming causal attention forward through the C ABI (csrc/attn_seq_long.hip: svla_attn_causal_fwd_bf16 via ops.attn_causal_fwd): query i of a row sees
keys j <= i of its own trajectory, up to 1024 keys.

Reference: the fp64 torch computation of tests/test_attn_decode_long_gpu.py (bf16-exact inputs, masked softmax, probabilities rounded to bf16 before P.V) with the
block-causal mask, computed once per (S, H, mask) and shared.  Gates: that file's own -- outputs close(1e-2, 1e-2), LSE allclose(1e-3, 1e-3) -- also against the two
kernels it borders on: the tile kernels of csrc/attn.hip at S <= 512 and one single-query row per position on ops.attn_decode_rows (the route it replaces)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROWS, HD, KT = 3, 64, 64                     # KT: the kernel's key tile (CSL_KT of csrc/attn_seq_long.hip)
SHAPES = [(513, 8), (513, 2), (1000, 8), (1024, 8), (9 * KT - 1, 8), (9 * KT, 8), (9 * KT + 1, 8), (1, 8), (17, 8)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from safevla_amd import ops as o

    return o


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


def close(got, want, rtol, atol, name=""):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    err = (got - want).abs()
    tol = atol + rtol * want.abs()
    print(f"{name}: max |err| {float(err.max()):.3e}, max err / tol {float((err / tol).max()):.3f}")
    assert torch.isfinite(got).all(), name
    assert not (err > tol).any(), (name, float(err.max()), float((err / tol).max()))


def _traj(S, kind):
    """[ROWS, S] int32 ids.  "equal": one trajectory.  "three": three trajectories per row whose boundaries differ per row -- row 0: one mid-tile, one exactly on a
    key-tile edge; row 1: both mid-tile; row 2: one on the first tile edge and a LAST trajectory of a single step."""
    if kind == "equal":
        return torch.full((ROWS, S), 7, dtype=torch.int32)
    if S >= 2 * KT + 2:
        bounds = [((S // 3) | 1, KT * ((2 * S // 3) // KT)), (37, S // 2 + 5), (KT, S - 1)]
    else:
        bounds = [(S // 3, 2 * S // 3), (S // 5, S - 1), (S // 2, S - 1)]
    t = torch.arange(S)
    return torch.stack([3 * sum(((t >= b).int() for b in bs if b > 0), torch.zeros(S, dtype=torch.int32)) + r for r, bs in enumerate(bounds)]).to(torch.int32)


_REF = {}


def _case(S, H, kind, seed=0):
    """fused qkv rows (bf16-exact fp32, CPU), the ids and the fp64 reference (computed on the device, kept on the CPU) of a case, computed once"""
    key = (S, H, kind, seed)
    if key not in _REF:
        D = H * HD
        qkv = rnd(ROWS * S, 3 * D, seed=311 + S + H + seed).bfloat16().float()
        traj = None if kind == "none" else _traj(S, kind)
        x = qkv.to(DEV).double().view(ROWS, S, 3, H, HD)
        sc = torch.einsum("rihd,rjhd->rhij", x[:, :, 0], x[:, :, 1]) * 0.125
        t = torch.arange(S, device=DEV)
        mask = (t[None, :] <= t[:, None])[None].expand(ROWS, S, S)
        if traj is not None:
            td = traj.to(DEV)
            mask = mask & (td[:, :, None] == td[:, None, :])
        sc = sc.masked_fill(~mask[:, None], float("-inf"))
        pu = torch.exp(sc - sc.max(-1, keepdim=True).values)
        den = pu.sum(-1)                                                    # [r, h, i]; a query sees itself: never 0
        want = torch.einsum("rhij,rjhd->rihd", pu.float().bfloat16().double(), x[:, :, 2]) / den.permute(0, 2, 1)[..., None]
        _REF[key] = dict(qkv=qkv, traj=traj, want=want.reshape(ROWS * S, D).cpu(), lse=torch.logsumexp(sc, -1).cpu())
        del sc, pu, mask
    return _REF[key]


@pytest.mark.parametrize("kind", ["none", "three"])
@pytest.mark.parametrize("S,H", SHAPES)
def test_causal_fwd_vs_fp64(ops, S, H, kind):
    D = H * HD
    c = _case(S, H, kind)
    qkv = c["qkv"].to(DEV).bfloat16()
    traj = None if c["traj"] is None else c["traj"].to(DEV)
    o, lse = ops.attn_causal_fwd(qkv, qkv[:, D:], qkv[:, 2 * D:], 3 * D, ROWS, S, H, 0.125, traj=traj, save_lse=True)
    o2, lse2 = ops.attn_causal_fwd(qkv, qkv[:, D:], qkv[:, 2 * D:], 3 * D, ROWS, S, H, 0.125, traj=traj, save_lse=False)
    torch.cuda.synchronize()
    name = f"causal S={S} H={H} traj={kind}"
    assert lse2 is None and torch.equal(o, o2), name                        # LSE on and off: the same outputs
    close(o.float(), c["want"], 1e-2, 1e-2, name + " vs fp64 torch")
    assert lse.shape == (ROWS, H, S)
    assert torch.allclose(lse.cpu().double(), c["lse"], rtol=1e-3, atol=1e-3), (name, float((lse.cpu().double() - c["lse"]).abs().max()))
    if kind == "none":                                                      # one trajectory per row is no trajectory mask: bit for bit
        o3, lse3 = ops.attn_causal_fwd(qkv, qkv[:, D:], qkv[:, 2 * D:], 3 * D, ROWS, S, H, 0.125, traj=_traj(S, "equal").to(DEV), save_lse=True)
        torch.cuda.synchronize()
        assert torch.equal(o, o3) and torch.equal(lse, lse3), name
    else:
        assert not torch.equal(o, ops.attn_causal_fwd(qkv, qkv[:, D:], qkv[:, 2 * D:], 3 * D, ROWS, S, H, 0.125)[0]) or S == 1, name


@pytest.mark.parametrize("S,H", [(513, 2), (1000, 8)])
def test_padded_strides(ops, S, H):
    """ld = 3 H 64 + 64 and a padded ldo give the outputs of the packed call, and the padding columns of the output keep their sentinel"""
    D = H * HD
    c = _case(S, H, "three")
    traj = c["traj"].to(DEV)
    packed = c["qkv"].to(DEV).bfloat16()
    want, want_lse = ops.attn_causal_fwd(packed, packed[:, D:], packed[:, 2 * D:], 3 * D, ROWS, S, H, 0.125, traj=traj, save_lse=True)
    wide = torch.full((ROWS * S, 3 * D + 64), 3.0, device=DEV, dtype=torch.bfloat16)
    wide[:, :3 * D] = packed
    out = torch.full((ROWS * S, D + 8), 7.0, device=DEV, dtype=torch.bfloat16)
    got, lse = ops.attn_causal_fwd(wide, wide[:, D:], wide[:, 2 * D:], 3 * D + 64, ROWS, S, H, 0.125, traj=traj, save_lse=True, out=out)
    torch.cuda.synchronize()
    assert got is out and torch.equal(out[:, :D], want) and (out[:, D:] == 7).all() and torch.equal(lse, want_lse)
    close(out[:, :D].float(), c["want"], 1e-2, 1e-2, f"padded S={S} H={H}")


@pytest.mark.parametrize("S", [512, 257])
def test_seam_against_the_tile_kernels(ops, S):
    """where both exist the two families are compared, not assumed equal: the online rescale changes the rounding"""
    H, D = 8, 512
    c = _case(S, H, "three")
    qkv, traj = c["qkv"].to(DEV).bfloat16(), c["traj"].to(DEV)
    o, lse = ops.attn_causal_fwd(qkv, qkv[:, D:], qkv[:, 2 * D:], 3 * D, ROWS, S, H, 0.125, traj=traj, save_lse=True)
    t, tlse = ops.attn_fwd(qkv, qkv[:, D:], qkv[:, 2 * D:], 3 * D, ROWS, S, H, 0.125, mask_mode=ops.MASK_BLOCK_CAUSAL, traj=traj, save_lse=True)
    torch.cuda.synchronize()
    close(o.float(), t.float(), 1e-2, 1e-2, f"seam S={S}: streaming vs tile kernel")
    close(o.float(), c["want"], 1e-2, 1e-2, f"seam S={S}: streaming vs fp64")
    close(t.float(), c["want"], 1e-2, 1e-2, f"seam S={S}: tile kernel vs fp64")
    assert torch.allclose(lse, tlse, rtol=1e-3, atol=1e-3)


def test_against_one_single_query_row_per_position(ops):
    """the route it replaces in the vector agent's window: ops.attn_decode_rows with rows * S query rows, klen = t + 1"""
    S, H, D = 600, 8, 512
    c = _case(S, H, "none")
    qkv = c["qkv"].to(DEV).bfloat16()
    o, lse = ops.attn_causal_fwd(qkv, qkv[:, D:], qkv[:, 2 * D:], 3 * D, ROWS, S, H, 0.125, save_lse=True)
    crow = torch.arange(ROWS, device=DEV, dtype=torch.int32).repeat_interleave(S)
    klen = (torch.arange(S, device=DEV) + 1).to(torch.int32).repeat(ROWS)
    d, dlse = ops.attn_decode_rows(qkv, 3 * D, qkv[:, D:], qkv[:, 2 * D:], 3 * D, klen, crow, ROWS * S, H, 0.125, S, save_lse=True)
    torch.cuda.synchronize()
    close(o.float(), d.float(), 1e-2, 1e-2, "S=600: streaming vs decode rows")
    assert torch.allclose(lse.permute(0, 2, 1).reshape(ROWS * S, H), dlse, rtol=1e-3, atol=1e-3)


def test_refusals_launch_nothing(ops):
    from safevla_amd._lib import SvlaError, lib

    H, S, D = 8, 600, 512
    qkv = rnd(ROWS * S, 3 * D, seed=5).bfloat16().to(DEV)
    st = torch.cuda.current_stream().cuda_stream
    NULL = object()

    def call(out, rows=ROWS, S=S, H=H, head_dim=64, ld=3 * D, ldo=D + 8, Q=qkv.data_ptr(), K=qkv[:, D:].data_ptr(), V=qkv[:, 2 * D:].data_ptr(), O=None):
        ptr = lambda v: None if v is NULL else v
        lib().call("svla_attn_causal_fwd_bf16", ptr(Q), ptr(K), ptr(V), ld, ptr(out.data_ptr() if O is None else O), ldo, None, rows, S, H, head_dim, 0.125, None, st)

    forms = {"head_dim 96": dict(head_dim=96), "head_dim 32": dict(head_dim=32), "rows = 0": dict(rows=0), "rows < 0": dict(rows=-1), "H = 0": dict(H=0),
             "H < 0": dict(H=-8), "S = 0": dict(S=0), "S < 0": dict(S=-5), "S = 1025": dict(S=1025), "ld % 8": dict(ld=3 * D + 4), "ld < H 64": dict(ld=D - 8),
             "ldo % 8": dict(ldo=D + 4), "ldo < H 64": dict(ldo=D - 8), "null Q": dict(Q=NULL), "null K": dict(K=NULL), "null V": dict(V=NULL), "null O": dict(O=NULL)}
    for name, kw in forms.items():
        out = torch.full((ROWS * S, D + 8), 7.0, device=DEV, dtype=torch.bfloat16)
        with pytest.raises(SvlaError, match="invalid argument"):
            call(out, **kw)
        torch.cuda.synchronize()
        assert (out == 7).all(), name
    out = torch.full((ROWS * S, D + 8), 7.0, device=DEV, dtype=torch.bfloat16)
    call(out)                                                               # the same call without a fault in it runs
    torch.cuda.synchronize()
    assert not (out[:, :D] == 7).any() and (out[:, D:] == 7).all()


def test_three_grouped_members_equal_three_single_launches(ops):
    """the kernel has a grouped twin: three members inside one launch-group capture are ONE grid, bit-identical to the launches alone"""
    import ctypes

    from safevla_amd import _lib

    H, D, S = 8, 512, 577
    qkv = [rnd(ROWS * S, 3 * D, seed=30 + m).bfloat16().to(DEV) for m in range(3)]
    traj = _traj(S, "three").to(DEV)
    call = lambda m: ops.attn_causal_fwd(qkv[m], qkv[m][:, D:], qkv[m][:, 2 * D:], 3 * D, ROWS, S, H, 0.125, traj=traj, save_lse=True)
    want = [call(m) for m in range(3)]
    ops.group_stats()
    L = _lib.lib()
    L.call("svla_group_begin", 3)
    try:
        got = []
        for m in range(3):
            L.call("svla_group_member", m)
            got.append(call(m))
    finally:
        rc = L.cdll.svla_group_end(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    grouped, alone = ops.group_stats()
    assert grouped >= 1 and alone == 0, (grouped, alone)
    for m in range(3):
        assert torch.equal(got[m][0], want[m][0]) and torch.equal(got[m][1], want[m][1]), m
    assert not torch.equal(got[0][0], got[1][0])
