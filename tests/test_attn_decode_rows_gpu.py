"""Per-row KV rings through the C ABI (csrc/attn_decode.hip): svla_attn_decode_rows_bf16 -- one query per row over the prefix [0, min(klen[r], kv_rows)) of
cache row cache_row[r] -- and svla_kv_append_rows_bf16 -- cache[cache_row[r], pos[r]] = src[r].

Reference of the attention: the fp64 torch computation of tests/test_attn_decode_long_gpu.py (from the same bf16 inputs, masked softmax, probabilities rounded to
bf16 before P.V) with a prefix mask, computed once per (window, heads, cache rows) and shared.  Gates: that file's own -- close(1e-2, 1e-2) against fp64,
(1e-2, 2e-3) against ops.attn_fwd(..., kvalid = prefix, Sq = 1, kv_rows = ...) on the same data, LSE at 1e-3, zero rows and a non-finite LSE where klen <= 0.
The append is compared bit for bit with a torch index_put over the whole cache."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROWS, HD, CACHE = 5, 64, 8
WINDOWS = [1, 31, 33, 512, 513, 1000, 1024]
PERM = [6, 2, 7, 0, 3]                       # row -> cache row of an 8-row cache


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


def _klens(W, shift):
    """per-row lengths of one call: 0, 1, 32, 33, W and W + 5 (clamped by the kernel) mixed, five of the six per call (``shift`` rotates which)"""
    vals = [0, 1, 32, 33, W, W + 5]
    return [vals[(r + shift) % 6] for r in range(ROWS)]


_REF = {}


def _case(W, H, permuted, shift):
    """inputs (bf16-exact fp32, CPU) and the fp64 reference of a case, computed once"""
    key = (W, H, permuted, shift)
    if key not in _REF:
        D = H * HD
        n_cache = CACHE if permuted else ROWS
        rows_of = PERM if permuted else list(range(ROWS))
        kv = rnd(n_cache * W, 2 * D, seed=171 + W + H).bfloat16().float()
        q = rnd(ROWS, 3 * D, seed=172 + W + H).bfloat16().float()           # ldq = 3 D: the query is the first third of a fused qkv row
        klen = _klens(W, shift)
        kvalid = torch.zeros(ROWS, W, dtype=torch.uint8)
        for r in range(ROWS):
            kvalid[r, :min(max(klen[r], 0), W)] = 1
        kv4 = kv.view(n_cache, W, 2 * D)[rows_of]                           # the cache rows the queries read, in query order
        K = kv4[:, :, :D].double().reshape(ROWS, W, H, HD)
        V = kv4[:, :, D:].double().reshape(ROWS, W, H, HD)
        sc = torch.einsum("rhd,rshd->rhs", q[:, :D].double().view(ROWS, H, HD), K) * 0.125
        sc = sc.masked_fill(~kvalid.bool()[:, None, :], float("-inf"))
        mx = sc.max(-1, keepdim=True).values
        mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
        pu = torch.exp(sc - mx)
        den = pu.sum(-1, keepdim=True)
        inv = torch.where(den > 0, 1.0 / den, torch.zeros_like(den))
        want = torch.einsum("rhs,rshd->rhd", pu.float().bfloat16().double(), V) * inv       # probabilities rounded to bf16 before P.V
        _REF[key] = dict(kv=kv, q=q, klen=klen, kvalid=kvalid, rows_of=rows_of, gathered=kv4.reshape(ROWS * W, 2 * D), lse=torch.logsumexp(sc, -1),
                         want=want.reshape(ROWS, D), empty=(den.squeeze(-1) == 0))
    return _REF[key]


@pytest.mark.parametrize("permuted", [False, True])
@pytest.mark.parametrize("H", [2, 8])
@pytest.mark.parametrize("W", WINDOWS)
def test_decode_rows_vs_fp64_and_the_kvalid_form(ops, W, H, permuted):
    D = H * HD
    for shift in (0, 3):                                                    # between them every length of the list, W + 5 included
        c = _case(W, H, permuted, shift)
        kv, q = c["kv"].to(DEV).bfloat16(), c["q"].to(DEV).bfloat16()
        klen = torch.tensor(c["klen"], dtype=torch.int32, device=DEV)
        crow = torch.tensor(c["rows_of"], dtype=torch.int32, device=DEV) if permuted else None
        o, lse = ops.attn_decode_rows(q, 3 * D, kv, kv[:, D:], 2 * D, klen, crow, ROWS, H, 0.125, W, save_lse=True)
        o2, lse2 = ops.attn_decode_rows(q, 3 * D, kv, kv[:, D:], 2 * D, klen, crow, ROWS, H, 0.125, W, save_lse=False)
        # the existing single-query kernels on the same keys: the cache rows gathered into query order, a prefix mask
        g = c["gathered"].to(DEV).bfloat16()
        o3, _ = ops.attn_fwd(q, g, g[:, D:], 2 * D, ROWS, W, H, 0.125, kvalid=c["kvalid"].to(DEV), save_lse=False, Sq=1, ldq=3 * D, kv_rows=W)
        torch.cuda.synchronize()
        name = f"decode rows W={W} H={H} perm={permuted} klen={c['klen']}"
        assert lse2 is None and torch.equal(o, o2), name
        close(o.float(), c["want"], 1e-2, 1e-2, name + " vs fp64 torch")
        close(o.float(), o3.float(), 1e-2, 2e-3, name + " vs attn_fwd with a prefix kvalid")
        empty = c["empty"]                                                  # [ROWS, H]
        got_lse = lse.view(ROWS, H).cpu()
        assert torch.allclose(got_lse[~empty].double(), c["lse"][~empty], rtol=1e-3, atol=1e-3), name
        if empty.any():
            assert (o.float().cpu().view(ROWS, H, HD)[empty] == 0).all(), name
            assert not torch.isfinite(got_lse[empty]).any(), name


@pytest.mark.parametrize("S", [33, 512, 513, 1024])
def test_a_prefix_gives_the_same_bits_through_every_kernel(ops, S):
    """The three kernels share their arithmetic (csrc/attn_decode.hip: the dec_* helpers) and add in the same order, so a prefix of n keys comes out bit for bit
    the same through attn_decode_rows (klen = n) and through attn_fwd with a prefix kvalid (S <= 512: attn_decode_kernel, above: attn_decode_long_kernel)."""
    rows, H = 4, 2
    D = H * HD
    kv, q = rnd(rows * S, 2 * D, seed=300 + S).bfloat16().to(DEV), rnd(rows, 3 * D, seed=301 + S).bfloat16().to(DEV)
    for n in (1, 32, 33, S):
        klen = torch.full((rows,), n, dtype=torch.int32, device=DEV)
        kvalid = torch.zeros(rows, S, dtype=torch.uint8, device=DEV)
        kvalid[:, :n] = 1
        o, lse = ops.attn_decode_rows(q, 3 * D, kv, kv[:, D:], 2 * D, klen, None, rows, H, 0.125, S, save_lse=True)
        o2, lse2 = ops.attn_fwd(q, kv, kv[:, D:], 2 * D, rows, S, H, 0.125, kvalid=kvalid, save_lse=True, Sq=1, ldq=3 * D, kv_rows=S)
        torch.cuda.synchronize()
        print(f"S={S} n={n}: max |dO| {float((o.float() - o2.float()).abs().max()):.3e}, max |dLSE| {float((lse.view(-1) - lse2.view(-1)).abs().max()):.3e}")
        assert torch.isfinite(lse).all() and (o.float().abs().sum(-1) > 0).all(), (S, n)
        assert torch.equal(o, o2), (S, n)
        assert torch.equal(lse.view(-1), lse2.view(-1)), (S, n)


def test_negative_klen_is_an_empty_row(ops):
    H, W, D = 2, 33, 128
    kv, q = rnd(ROWS * W, 2 * D, seed=1).bfloat16().to(DEV), rnd(ROWS, 3 * D, seed=2).bfloat16().to(DEV)
    klen = torch.tensor([-3, 5, 0, -1, 33], dtype=torch.int32, device=DEV)
    o, lse = ops.attn_decode_rows(q, 3 * D, kv, kv[:, D:], 2 * D, klen, None, ROWS, H, 0.125, W, save_lse=True)
    torch.cuda.synchronize()
    assert (o[[0, 2, 3]] == 0).all() and not torch.isfinite(lse[[0, 2, 3]]).any()
    assert torch.isfinite(lse[[1, 4]]).all() and (o[[1, 4]].float().abs().sum(-1) > 0).all()


def test_refusals_launch_nothing(ops):
    from safevla_amd._lib import SvlaError, lib

    H, W, D = 8, 600, 512
    kv, q = rnd(ROWS * W, 2 * D, seed=3).bfloat16().to(DEV), rnd(ROWS, 3 * D, seed=4).bfloat16().to(DEV)
    klen = torch.full((ROWS,), W, dtype=torch.int32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def call(out, rows=ROWS, H=H, head_dim=64, kv_rows=W, ld=2 * D, ldq=3 * D, ldo=D, klen_p=klen.data_ptr()):
        lib().call("svla_attn_decode_rows_bf16", q.data_ptr(), ldq, kv.data_ptr(), kv[:, D:].data_ptr(), ld, out.data_ptr(), ldo, None, klen_p, None, rows, H, head_dim,
                   0.125, kv_rows, st)

    forms = {"rows = 0": dict(rows=0), "rows < 0": dict(rows=-1), "H = 0": dict(H=0), "head_dim 96": dict(head_dim=96), "head_dim 32": dict(head_dim=32),
             "kv_rows = 0": dict(kv_rows=0), "kv_rows = 1025": dict(kv_rows=1025), "ld % 8": dict(ld=2 * D + 4), "ldq % 8": dict(ldq=3 * D + 2),
             "ldo % 8": dict(ldo=D + 4), "null klen": dict(klen_p=None)}
    for name, kw in forms.items():
        out = torch.full((ROWS, D + 8), 7.0, device=DEV, dtype=torch.bfloat16)
        with pytest.raises(SvlaError, match="invalid argument"):
            call(out, **kw)
        torch.cuda.synchronize()
        assert (out == 7).all(), name
    out = torch.full((ROWS, D), 7.0, device=DEV, dtype=torch.bfloat16)
    call(out)                                                               # the same call without a fault in it runs
    torch.cuda.synchronize()
    assert not (out == 7).any()


@pytest.mark.parametrize("permuted", [False, True])
@pytest.mark.parametrize("width", [1024, 1536])
def test_kv_append_rows_equals_index_put_over_the_whole_cache(ops, width, permuted):
    slots = 40
    n_cache = CACHE if permuted else ROWS
    ld_src = 3 * width // 2
    src = rnd(ROWS, ld_src, seed=width).bfloat16().to(DEV)
    cache = rnd(n_cache, slots, width, seed=width + 1).bfloat16().to(DEV)
    pos = [3, -1, 39, 0, 17]                                                # row 1 is skipped
    rows_of = PERM if permuted else list(range(ROWS))
    want = cache.clone()
    keep = [r for r in range(ROWS) if pos[r] >= 0]
    want.index_put_((torch.tensor([rows_of[r] for r in keep], device=DEV), torch.tensor([pos[r] for r in keep], device=DEV)), src[keep, :width])
    crow = torch.tensor(rows_of, dtype=torch.int32, device=DEV) if permuted else None
    ops.kv_append_rows(src, ld_src, cache, crow, torch.tensor(pos, dtype=torch.int32, device=DEV), ROWS, width)
    torch.cuda.synchronize()
    assert torch.equal(cache.view(torch.int16), want.view(torch.int16))     # every cell, the untouched ones included
    assert not torch.equal(cache[rows_of[0], 3], cache[rows_of[3], 0])


def test_kv_append_rows_refusals(ops):
    from safevla_amd._lib import SvlaError

    src, cache = torch.zeros(ROWS, 64, device=DEV, dtype=torch.bfloat16), torch.full((ROWS, 4, 64), 7.0, device=DEV, dtype=torch.bfloat16)
    pos = torch.zeros(ROWS, dtype=torch.int32, device=DEV)
    for kw in (dict(rows=0, width=64, ld_src=64), dict(rows=ROWS, width=60, ld_src=64), dict(rows=ROWS, width=64, ld_src=68)):
        with pytest.raises(SvlaError, match="invalid argument"):
            ops.kv_append_rows(src, kw["ld_src"], cache, None, pos, kw["rows"], kw["width"])
    torch.cuda.synchronize()
    assert (cache == 7).all()


def test_three_grouped_members_equal_three_single_launches(ops):
    """both kernels have a grouped twin: three members inside one launch-group capture are ONE grid each, bit-identical to the launches alone"""
    import ctypes

    from safevla_amd import _lib

    H, D, W = 8, 512, 100
    kv = [rnd(ROWS * W, 2 * D, seed=10 + m).bfloat16().to(DEV) for m in range(3)]
    q = [rnd(ROWS, 3 * D, seed=20 + m).bfloat16().to(DEV) for m in range(3)]
    klen = torch.tensor([1, 40, 100, 64, 7], dtype=torch.int32, device=DEV)
    pos = torch.tensor([0, 39, 99, -1, 6], dtype=torch.int32, device=DEV)

    def call(m, caches):
        ops.kv_append_rows(q[m][:, D:], 3 * D, caches[m].view(ROWS, W, 2 * D), None, pos, ROWS, 2 * D)
        return ops.attn_decode_rows(q[m], 3 * D, caches[m], caches[m][:, D:], 2 * D, klen, None, ROWS, H, 0.125, W, save_lse=True)

    single = [t.clone() for t in kv]
    want = [call(m, single) for m in range(3)]
    ops.group_stats()
    L = _lib.lib()
    L.call("svla_group_begin", 3)
    try:
        got = []
        for m in range(3):
            L.call("svla_group_member", m)
            got.append(call(m, kv))
    finally:
        rc = L.cdll.svla_group_end(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    grouped, alone = ops.group_stats()
    assert grouped >= 2 and alone == 0, (grouped, alone)
    for m in range(3):
        assert torch.equal(got[m][0], want[m][0]) and torch.equal(got[m][1], want[m][1]) and torch.equal(kv[m], single[m]), m
    assert not torch.equal(got[0][0], got[1][0])
