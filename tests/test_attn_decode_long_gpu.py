"""Single-query ("decode") attention over a KV-cache window of 512 < S <= 1024 keys (csrc/attn_decode.hip behind svla_attn_fwd_bf16, its fp32 twin behind
svla_attn_fwd_f32): the acting step of the llama decoder on episodes of up to 1000 steps, the length the reference's online evaluation runs.

Reference: fp64 torch on the CPU from the same bf16 inputs, masked softmax over ``kvalid``, probabilities rounded to bf16 before P.V (the kernel's arithmetic:
bf16 products, fp32 accumulation).  Gates: those of tests/test_kernels_gpu.py::test_attn_single_query_decode_kernel -- close(1e-2, 1e-2) against torch,
(1e-2, 2e-3) against the other kernel, LSE at 1e-3 against logsumexp; the fp32 twin at the 2e-5 (max error relative to the largest value) of
tests/test_fp32_mode_gpu.py."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROWS, HD = 3, 64


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


def _kvalid(S, spec):
    """[ROWS, S] uint8 or None.  A (lo, hi) pair: the contiguous window of an episode that began at slot lo (row r starts r slots later, like envs that restarted
    at different steps)."""
    if spec is None:
        return None
    kv = torch.zeros(ROWS, S, dtype=torch.uint8)
    if spec == "all":
        kv[:] = 1
    elif spec == "scattered":
        kv[:] = (torch.rand(ROWS, S, generator=torch.Generator().manual_seed(S)) < 0.3).to(torch.uint8)
        kv[0, S - 1] = 1
    elif spec == "one_none_window":
        kv[0, 640] = 1                      # a single valid key; row 1: none at all
        kv[2, 100:S - 7] = 1
    else:
        lo, hi = spec
        for r in range(ROWS):
            kv[r, min(lo + r, hi):hi + 1] = 1
    return kv


# (S, kv_rows, H, kvalid): 513 = the smallest new shape (one key in the last block); 1000 = the reference's window; 1024 = the limit; 777 / 1000 / 513 are no
# multiples of 32; windows that start late and one across the old limit of 512; single key / no key; scattered masks
CASES = [(513, 513, 8, None), (513, 600, 2, "all"), (1000, 1000, 8, None), (1024, 1024, 8, None), (777, 1000, 8, "scattered"), (1024, 1024, 2, "scattered"),
         (1000, 1000, 8, (700, 999)), (514, 1000, 8, (511, 513)), (1000, 1024, 2, "one_none_window"), (600, 1000, 8, (0, 599))]
_REF = {}


def _case(S, kv_rows, H, spec):
    """inputs (bf16-exact fp32, CPU) and the fp64 references of a case, computed once and shared by the bf16 and the fp32 tests"""
    key = (S, kv_rows, H, str(spec))
    if key not in _REF:
        D = H * HD
        kv = rnd(ROWS * kv_rows, 2 * D, seed=71 + S).bfloat16().float()
        q = rnd(ROWS, 3 * D, seed=72 + S).bfloat16().float()               # ldq = 3 D: the query is the first third of a fused qkv row
        kvalid = _kvalid(S, spec)
        K = kv[:, :D].double().view(ROWS, kv_rows, H, HD)[:, :S]
        V = kv[:, D:].double().view(ROWS, kv_rows, H, HD)[:, :S]
        sc = torch.einsum("rhd,rshd->rhs", q[:, :D].double().view(ROWS, H, HD), K) * 0.125
        if kvalid is not None:
            sc = sc.masked_fill(~kvalid.bool()[:, None, :], float("-inf"))
        mx = sc.max(-1, keepdim=True).values
        mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
        pu = torch.exp(sc - mx)                                             # unnormalised probabilities, 0 where masked
        den = pu.sum(-1, keepdim=True)
        inv = torch.where(den > 0, 1.0 / den, torch.zeros_like(den))
        want_bf = torch.einsum("rhs,rshd->rhd", pu.float().bfloat16().double(), V) * inv          # probabilities rounded to bf16 before P.V
        want_f32 = torch.einsum("rhs,rshd->rhd", pu, V) * inv
        _REF[key] = dict(kv=kv, q=q, kvalid=kvalid, lse=torch.logsumexp(sc, -1), want_bf=want_bf.reshape(ROWS, D), want_f32=want_f32.reshape(ROWS, D),
                         empty=(den.squeeze(-1) == 0))
    return _REF[key]


@pytest.mark.parametrize("S,kv_rows,H,spec", CASES)
def test_long_window_decode_bf16(ops, S, kv_rows, H, spec):
    c = _case(S, kv_rows, H, spec)
    D = H * HD
    kv, q = c["kv"].to(DEV).bfloat16(), c["q"].to(DEV).bfloat16()
    kvalid = None if c["kvalid"] is None else c["kvalid"].to(DEV)
    o, lse = ops.attn_fwd(q, kv, kv[:, D:], 2 * D, ROWS, S, H, 0.125, kvalid=kvalid, save_lse=True, Sq=1, ldq=3 * D, kv_rows=kv_rows)
    o2, lse2 = ops.attn_fwd(q, kv, kv[:, D:], 2 * D, ROWS, S, H, 0.125, kvalid=kvalid, save_lse=False, Sq=1, ldq=3 * D, kv_rows=kv_rows)
    torch.cuda.synchronize()
    assert lse2 is None and torch.equal(o, o2)
    close(o.float(), c["want_bf"], 1e-2, 1e-2, f"long decode S={S} H={H} {spec} vs fp64 torch")
    empty = c["empty"]                                                       # [ROWS, H]
    got_lse = lse.view(ROWS, H).cpu()
    assert torch.allclose(got_lse[~empty].double(), c["lse"][~empty], rtol=1e-3, atol=1e-3)
    if empty.any():
        assert (o.float().cpu().view(ROWS, H, HD)[empty] == 0).all()         # a row without a valid key: zeros ...
        assert not torch.isfinite(got_lse[empty]).any()                      # ... and the log of an empty sum, as attn_decode_kernel reports it


@pytest.mark.parametrize("S,kv_rows,H,spec", CASES)
def test_long_window_decode_fp32_twin(ops, S, kv_rows, H, spec):
    c = _case(S, kv_rows, H, spec)
    D = H * HD
    kv, q = c["kv"].to(DEV), c["q"].to(DEV)
    kvalid = None if c["kvalid"] is None else c["kvalid"].to(DEV)
    o, lse = ops.attn_fwd(q, kv, kv[:, D:], 2 * D, ROWS, S, H, 0.125, kvalid=kvalid, save_lse=True, Sq=1, ldq=3 * D, kv_rows=kv_rows)
    torch.cuda.synchronize()
    assert o.dtype == torch.float32
    want = c["want_f32"]
    err = float((o.double().cpu() - want).abs().max() / (want.abs().max() + 1e-30))
    print(f"fp32 twin S={S} H={H} {spec}: max error relative to the largest value {err:.3e}")
    assert torch.isfinite(o).all() and err < 2e-5
    empty = c["empty"]
    got_lse = lse.view(ROWS, H).cpu()
    assert float((got_lse[~empty].double() - c["lse"][~empty]).abs().max() / c["lse"][~empty].abs().max()) < 2e-5
    if empty.any():
        assert (o.cpu().view(ROWS, H, HD)[empty] == 0).all() and (got_lse[empty] == float("-inf")).all()


def test_continuous_with_the_512_key_kernel_at_the_old_limit(ops):
    """The same data truncated to S = 512 on the existing kernel, and at S = 513 with key 512 masked on the new one: the same keys, so the same output within the
    'decode kernel vs tile kernel' gate of test_attn_single_query_decode_kernel."""
    H, D, cap = 8, 512, 600
    kv = rnd(ROWS * cap, 2 * D, seed=5).bfloat16().to(DEV)
    q = rnd(ROWS, 3 * D, seed=6).bfloat16().to(DEV)
    for lo in (0, 300):
        kva = torch.zeros(ROWS, 513, dtype=torch.uint8, device=DEV)
        kva[:, lo:512] = 1
        o_old, l_old = ops.attn_fwd(q, kv, kv[:, D:], 2 * D, ROWS, 512, H, 0.125, kvalid=kva[:, :512].contiguous(), save_lse=True, Sq=1, ldq=3 * D, kv_rows=cap)
        o_new, l_new = ops.attn_fwd(q, kv, kv[:, D:], 2 * D, ROWS, 513, H, 0.125, kvalid=kva, save_lse=True, Sq=1, ldq=3 * D, kv_rows=cap)
        torch.cuda.synchronize()
        close(o_new.float(), o_old.float(), 1e-2, 2e-3, f"S = 513 with key 512 masked vs S = 512, window from {lo}")
        assert torch.allclose(l_new, l_old, rtol=1e-4, atol=1e-4)


def test_every_other_form_above_512_keys_is_refused_and_launches_nothing(ops):
    from safevla_amd._lib import SvlaError, lib

    H, D, S = 8, 512, 600
    kv = rnd(ROWS * 1025, 2 * D, seed=1).bfloat16().to(DEV)
    q = rnd(ROWS, 3 * D, seed=2).bfloat16().to(DEV)
    traj = torch.zeros(ROWS, S, dtype=torch.int32, device=DEV)
    kw = dict(save_lse=False, Sq=1, ldq=3 * D)
    forms = {
        "S = 1025": lambda out: ops.attn_fwd(q, kv, kv[:, D:], 2 * D, ROWS, 1025, H, 0.125, out=out, **kw),
        "dropout": lambda out: ops.attn_fwd(q, kv, kv[:, D:], 2 * D, ROWS, S, H, 0.125, drop=ops.Dropout(3, 1, 0.1), out=out, **kw),
        "block-causal": lambda out: ops.attn_fwd(q, kv, kv[:, D:], 2 * D, ROWS, S, H, 0.125, mask_mode=ops.MASK_BLOCK_CAUSAL, traj=traj, out=out, **kw),
        "all queries": lambda out: ops.attn_fwd(kv, kv[:, D:], kv[:, D:], 2 * D, 1, S, H, 0.125, save_lse=False, out=None),
    }
    for name, fn in forms.items():
        out = torch.full((ROWS, D), 7.0, device=DEV, dtype=torch.bfloat16)
        with pytest.raises(SvlaError):
            fn(out)
        torch.cuda.synchronize()
        assert (out == 7).all(), name
    # heads of 96: the bf16 entry point itself, and ops.attn_fwd (whose route for S > 256 is the fp32 kernels: those stop at 512 keys for this width)
    H96 = 4
    kv96 = rnd(ROWS * S, 2 * H96 * 96, seed=3).bfloat16().to(DEV)
    q96 = rnd(ROWS, H96 * 96, seed=4).bfloat16().to(DEV)
    out = torch.full((ROWS, H96 * 96), 7.0, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(SvlaError):
        lib().call("svla_attn_fwd_bf16", q96.data_ptr(), kv96.data_ptr(), kv96[:, H96 * 96:].data_ptr(), 2 * H96 * 96, out.data_ptr(), H96 * 96, None, ROWS, S, H96, 96,
                   96 ** -0.5, 0, None, None, None, 1, H96 * 96, S, None, torch.cuda.current_stream().cuda_stream)
    with pytest.raises(SvlaError):
        ops.attn_fwd(q96, kv96, kv96[:, H96 * 96:], 2 * H96 * 96, ROWS, S, H96, 96 ** -0.5, save_lse=False, Sq=1, ldq=H96 * 96, head_dim=96, out=out)
    torch.cuda.synchronize()
    assert (out == 7).all()
    # the tile-kernel hook (single-query forwards on the tile kernels) has no kernel above 512 keys either
    lib().call("svla_attn_bwd_two_pass", 4)
    try:
        out = torch.full((ROWS, D), 7.0, device=DEV, dtype=torch.bfloat16)
        with pytest.raises(SvlaError):
            ops.attn_fwd(q, kv, kv[:, D:], 2 * D, ROWS, S, H, 0.125, out=out, **kw)
        torch.cuda.synchronize()
        assert (out == 7).all()
    finally:
        lib().call("svla_attn_bwd_two_pass", 0)


def _grouped(fn_per_member, members=3):
    """run fn_per_member(m) for m in range(members) inside one launch-group capture on the current stream"""
    from safevla_amd import _lib

    L = _lib.lib()
    L.call("svla_group_begin", members)
    try:
        outs = []
        for m in range(members):
            L.call("svla_group_member", m)
            outs.append(fn_per_member(m))
    finally:
        rc = L.cdll.svla_group_end(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    return outs


def test_three_grouped_members_equal_three_single_launches(ops):
    """three 'towers' on the new shape in one launch-group capture: ONE grid of the grouped twin, bit-identical to the three launches alone"""
    H, D, S, cap = 8, 512, 1000, 1000
    kv = [rnd(ROWS * cap, 2 * D, seed=10 + m).bfloat16().to(DEV) for m in range(3)]
    q = [rnd(ROWS, 3 * D, seed=20 + m).bfloat16().to(DEV) for m in range(3)]
    kvalid = _kvalid(S, (397, 640)).to(DEV)
    call = lambda m: ops.attn_fwd(q[m], kv[m], kv[m][:, D:], 2 * D, ROWS, S, H, 0.125, kvalid=kvalid, save_lse=True, Sq=1, ldq=3 * D, kv_rows=cap)
    want = [call(m) for m in range(3)]
    ops.group_stats()
    got = _grouped(call)
    torch.cuda.synchronize()
    grouped, single = ops.group_stats()
    assert grouped >= 1 and single == 0, (grouped, single)
    for m in range(3):
        assert torch.equal(got[m][0], want[m][0]) and torch.equal(got[m][1], want[m][1]), m
    assert not torch.equal(got[0][0], got[1][0])
