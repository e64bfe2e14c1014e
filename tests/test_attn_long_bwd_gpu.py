"""bf16 attention backward for 64-wide heads and 256 < S <= 512 (csrc/attn_long.hip) against an fp64 torch reference, through ``ops.attn_bwd`` and the C ABI,
through ``EarlyFusionCnnTransformer`` on a whole 272-step episode and through one PPO-Lagrangian accumulation over a 320-step rollout.  Before these kernels
existed every backward above 256 keys raised ``SvlaError`` (invalid argument): tests 1, 6 and 7 fail that way without them.

Gates are the ones the S <= 256 kernels are held to, none was widened:
  * gradients vs fp64 (tests/test_kernels_gpu.py::_attn_case): ``close(rtol 2e-2, atol 2e-2 * max|want| + 1e-3)``, forward output ``close(1e-2, 1e-2)``;
  * continuity S = 256 (shipped kernel) vs S = 257 with the extra key masked: one bf16 ulp of the output (rtol 2^-7) plus half an ulp of the largest
    gradient element (atol 2^-8 max|want|): both kernels round the same fp32 sums, up to the order of the additions and a flipped bf16 rounding of single
    probabilities, each worth at most 2^-8 of ONE of the S terms of a sum;
  * whole-episode imitation learning vs the CPU oracle (tests/test_il_gpu.py::test_other_model_versions_vs_oracle): logits / loss 3e-2, parameter-gradient relative L2
    median 6e-2, max 0.2;
  * PPO-Lagrangian accumulation, bf16 vs the fp32 verification mode (tests/test_fp32_mode_gpu.py::test_bf16_product_path_vs_fp32_mode_at_a_size_the_cpu_oracle_cannot_reach):
    loss sums rtol 1e-2, gradient cosine > 0.9999, relative L2 < 1.5e-2, per-tower cosine > 0.998.
Every case prints its worst error before it asserts."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
HD = 64
SCALE = 0.125
LONG_S = [257, 272, 289, 300, 433, 448, 449, 500, 512]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from safevla_amd import ops as o

    return o


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(torch.bfloat16).float()      # bf16-exact fp32 values


def close(got, want, rtol, atol, name):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert torch.isfinite(got).all(), name
    err = (got - want).abs()
    print(f"    {name}: worst abs error {err.max().item():.3e} ({err.max().item() / (want.abs().max().item() + 1e-30):.3e} of max|want| = {want.abs().max().item():.3f})")
    bad = err > atol + rtol * want.abs()
    assert not bad.any(), (name, int(bad.sum()), err.max().item())


def hash_mask(seed, stream, p, rows, H, nq, S):
    """keep-mask [rows, H, nq, S] of the attention-probability dropout: element index ((r*H + h)*S + q) * S4 + k (include/svla.h: svla_dropout)"""
    from oracle.ref_model import hash_keep

    S4 = (S + 3) & ~3
    idx = ((np.arange(rows * H, dtype=np.uint64)[:, None, None] * np.uint64(S) + np.arange(nq, dtype=np.uint64)[None, :, None]) * np.uint64(S4)
           + np.arange(S, dtype=np.uint64)[None, None, :]).reshape(rows, H, nq, S)
    return torch.from_numpy(hash_keep(seed, stream, p, idx))


def ref_attn(q, k, v, mask=None, keep=None, p=0.0):
    """fp64 reference: q [rows, H, nq, 64], k / v [rows, H, S, 64]; mask broadcastable to [rows, H, nq, S] (True = attend).  A query without any
    visible key gets a zero output (and zero gradients), as the kernels define it."""
    s = (q @ k.transpose(-1, -2)) * SCALE
    if mask is not None:
        alive = mask.any(-1, keepdim=True)
        s = s.masked_fill(~(mask | ~alive), float("-inf"))
        pr = torch.softmax(s, -1) * alive
    else:
        pr = torch.softmax(s, -1)
    if keep is not None:
        pr = pr * keep / (1.0 - float(np.float32(p)))
    return pr @ v


def run_case(ops, S, H=8, rows=2, Sq=0, mask_mode=0, traj=None, kvalid=None, p=0.0, seed=0, d_ws="auto", name=""):
    """one forward + backward through ops.attn_fwd / ops.attn_bwd against the fp64 reference; returns (dQ, dK, dV, fp64 leaves)"""
    W = H * HD
    nq = Sq or S
    heads = lambda t, n: t.view(rows, n, H, HD).transpose(1, 2).double().clone().requires_grad_(True)
    kv, qs = rnd(rows * S, 2 * W, seed=seed + 1), rnd(rows * nq, W, seed=seed + 2)
    k, v, q = heads(kv[:, :W], S), heads(kv[:, W:], S), heads(qs, nq)
    mask = None
    if mask_mode == 1:
        mask = torch.tril(traj[:, :, None] == traj[:, None, :])[:, None, :nq]
    if kvalid is not None:
        km = kvalid.bool()[:, None, None, :]
        mask = km if mask is None else (mask & km)
    drop, keep = None, None
    if p > 0:
        drop = ops.Dropout(seed=0xBEEF, stream=4, p=p)
        keep = hash_mask(0xBEEF, 4, p, rows, H, nq, S)
    want = ref_attn(q, k, v, mask, keep, p)
    kw = dict(mask_mode=mask_mode, traj=None if traj is None else traj.int().to(DEV), kvalid=None if kvalid is None else kvalid.to(torch.uint8).to(DEV), drop=drop)
    d_kv, d_q = kv.to(DEV).bfloat16(), qs.to(DEV).bfloat16()
    if Sq:
        out, lse = ops.attn_fwd(d_q, d_kv, d_kv[:, W:], 2 * W, rows, S, H, SCALE, Sq=Sq, ldq=W, **kw)
    else:      # all queries: q laid out like k / v (one fused tensor)
        qkv = torch.cat([d_q, d_kv], 1)
        out, lse = ops.attn_fwd(qkv, qkv[:, W:], qkv[:, 2 * W:], 3 * W, rows, S, H, SCALE, **kw)
    close(out.float().view(rows, nq, H, HD), want.transpose(1, 2), 1e-2, 1e-2, f"{name} O")
    do = rnd(rows * nq, W, seed=seed + 5)
    want.backward(do.view(rows, nq, H, HD).transpose(1, 2).double())
    d_do = do.to(DEV).bfloat16()
    if d_ws == "given":
        kw["d_ws"] = torch.zeros(rows * H * nq, device=DEV)
    if Sq:
        dq, dkv = torch.full_like(d_q, 7.0), torch.full_like(d_kv, 7.0)
        ops.attn_bwd(d_q, d_kv, d_kv[:, W:], 2 * W, out, W, lse, d_do, W, dq, dkv, dkv[:, W:], 2 * W, rows, S, H, SCALE, Sq=Sq, ldq=W, lddq=W, **kw)
        got = [dq.view(rows, nq, H, HD), dkv[:, :W].view(rows, S, H, HD), dkv[:, W:].view(rows, S, H, HD)]
    else:
        dqkv = torch.full_like(qkv, 7.0)
        ops.attn_bwd(qkv, qkv[:, W:], qkv[:, 2 * W:], 3 * W, out, W, lse, d_do, W, dqkv, dqkv[:, W:], dqkv[:, 2 * W:], 3 * W, rows, S, H, SCALE, **kw)
        got = [dqkv[:, i * W:(i + 1) * W].view(rows, S, H, HD) for i in range(3)]
    for g_, t, n in zip(got, (q, k, v), ("dQ", "dK", "dV")):
        w = t.grad.transpose(1, 2)
        close(g_.float(), w, 2e-2, 2e-2 * w.abs().max().item() + 1e-3, f"{name} {n}")
    return got, (q, k, v)


def ragged_traj(rows, S, seed):
    """several trajectories per row, boundaries at random steps (the last one ends ragged at the window's end)"""
    g = torch.Generator().manual_seed(seed)
    return torch.cumsum((torch.rand(rows, S, generator=g) < 0.02).long(), dim=1) + 3


# ------------------------------------------------------------------------------------------------ 1. every long length, no mask
@pytest.mark.parametrize("S", LONG_S)
def test_bwd_long_lengths_vs_fp64(ops, S):
    """the forward's own long-S list plus the episode length; each raised SvlaError before csrc/attn_long.hip"""
    run_case(ops, S, H=8, rows=2, seed=S, name=f"S={S}")


def test_c_abi_direct_with_and_without_d_ws(ops):
    """svla_attn_bwd_bf16 called directly at S = 300, ``D_ws`` null and given"""
    from safevla_amd._lib import lib

    rows, S, H = 2, 300, 8
    W = H * HD
    qkv = rnd(rows * S, 3 * W, seed=1)
    heads = lambda t: t.view(rows, S, H, HD).transpose(1, 2).double().clone().requires_grad_(True)
    q, k, v = heads(qkv[:, :W]), heads(qkv[:, W:2 * W]), heads(qkv[:, 2 * W:])
    want = ref_attn(q, k, v)
    d = qkv.to(DEV).bfloat16()
    out, lse = ops.attn_fwd(d, d[:, W:], d[:, 2 * W:], 3 * W, rows, S, H, SCALE)
    do = rnd(rows * S, W, seed=2)
    want.backward(do.view(rows, S, H, HD).transpose(1, 2).double())
    d_do = do.to(DEV).bfloat16()
    p_, st = ops._p, ops._stream()
    res = []
    for d_ws in (None, torch.zeros(rows * H * S, device=DEV)):
        dd = torch.full_like(d, 7.0)
        lib().call("svla_attn_bwd_bf16", p_(d), p_(d[:, W:]), p_(d[:, 2 * W:]), 3 * W, p_(out), W, p_(lse), p_(d_do), W, p_(dd), p_(dd[:, W:]), p_(dd[:, 2 * W:]), 3 * W,
                   rows, S, H, 64, float(SCALE), 0, None, None, None, 0, 0, 0, p_(d_ws), None, st)
        for i, (n, t) in enumerate((("dQ", q), ("dK", k), ("dV", v))):
            w = t.grad.transpose(1, 2)
            close(dd[:, i * W:(i + 1) * W].float().view(rows, S, H, HD), w, 2e-2, 2e-2 * w.abs().max().item() + 1e-3, f"C ABI {n} (D_ws {'given' if d_ws is not None else 'null'})")
        res.append(dd)
    assert torch.equal(res[0], res[1])


# ------------------------------------------------------------------------------------------------ 2. the mode table
@pytest.mark.parametrize("S", [300, 500])
def test_mode_table(ops, S):
    rows = 2
    for H in (2, 12):
        run_case(ops, S, H=H, rows=rows, seed=10 + H, name=f"S={S} H={H}")
    run_case(ops, S, H=8, rows=rows, d_ws="given", seed=3, name=f"S={S} D_ws given")
    # block-causal, several trajectories per row, ragged ends
    for H in (2, 8, 12):
        run_case(ops, S, H=H, rows=rows, mask_mode=1, traj=ragged_traj(rows, S, S + H), seed=20 + H, name=f"S={S} H={H} block-causal")
    # query subsets
    for Sq in (1, 17):
        run_case(ops, S, H=8, rows=rows, Sq=Sq, seed=30 + Sq, name=f"S={S} Sq={Sq}")
        run_case(ops, S, H=8, rows=rows, Sq=Sq, mask_mode=1, traj=ragged_traj(rows, S, 5), seed=40 + Sq, name=f"S={S} Sq={Sq} block-causal")
    # key padding alone: a ragged row and a row with a single valid key
    kvalid = torch.ones(rows, S)
    kvalid[0, S - 57:] = 0
    kvalid[1, 1:] = 0
    run_case(ops, S, H=8, rows=rows, kvalid=kvalid, seed=50, name=f"S={S} kvalid")


@pytest.mark.parametrize("S", [300, 500])
def test_kvalid_with_fully_masked_keys_and_a_fully_masked_query(ops, S):
    """block-causal + key padding with key 0 of row 1 invalid: query 0 of that row sees no key at all -- its dQ is exactly 0, masked keys get exactly 0, nothing is NaN"""
    rows, H = 2, 8
    traj = torch.zeros(rows, S, dtype=torch.long)
    traj[0, 200:] = 1
    kvalid = torch.ones(rows, S)
    kvalid[0, 280:] = 0
    kvalid[1, 0] = 0
    kvalid[1, 100:140] = 0
    got, _ = run_case(ops, S, H=H, rows=rows, mask_mode=1, traj=traj, kvalid=kvalid, seed=60, name=f"S={S} kvalid + block-causal")
    dq, dk, dv = [g.float().cpu() for g in got]
    assert bool((dq[1, 0] == 0).all())
    for t in (dk, dv):
        assert bool((t[0, 280:] == 0).all()) and bool((t[1, 0] == 0).all()) and bool((t[1, 100:140] == 0).all())


@pytest.mark.parametrize("S,causal", [(300, False), (300, True), (500, True)])
def test_dropout_vs_fp64_with_the_counter_mask(ops, S, causal):
    run_case(ops, S, H=8, rows=2, mask_mode=int(causal), traj=ragged_traj(2, S, 7) if causal else None, p=0.1, seed=70, name=f"S={S} dropout{' block-causal' if causal else ''}")
    if not causal:
        run_case(ops, S, H=8, rows=2, Sq=17, p=0.1, seed=71, name=f"S={S} Sq=17 dropout")


def test_dropout_mask_bits_forward_dq_kernel_and_dkv_kernel_agree(ops):
    """S = 300, p = 0.1, Q = 0 (uniform probabilities 1/S): every keep bit of the forward, of the dQ kernel and of the dK/dV kernel is read back and compared with the
    counter definition, 64 keys (queries) at a time through one-hot operands:
      forward    V = one-hot on a key chunk              => O[q, d]  != 0            <=> keep[q, chunk + d]
      dK/dV      dO = one-hot on a query chunk           => dV[k, d] != 0            <=> keep[chunk + d, k]
      dQ         K one-hot on a key chunk, V = v_k e_0, dO = e_0, v_k = +-4: dS[q, k] = (keep v_k / 0.9 - D_q) / S with |D_q| < 2, so
                 |dQ[q, d] S / scale + D_q| > 2                                      <=> keep[q, chunk + d]"""
    rows, H, S, p = 1, 2, 300, 0.1
    W = H * HD
    drop = ops.Dropout(seed=0xBEEF, stream=4, p=p)
    keep = hash_mask(0xBEEF, 4, p, rows, H, S, S).bool()[0]      # [H, q, k]
    assert 0.05 < 1.0 - keep.float().mean().item() < 0.15
    fwd_bits, dkv_bits, dq_bits = torch.zeros_like(keep), torch.zeros_like(keep), torch.zeros_like(keep)
    sign = torch.where(torch.rand(S, generator=torch.Generator().manual_seed(5)) < 0.5, -4.0, 4.0)
    for c0 in range(0, S, HD):
        n = min(HD, S - c0)
        hot = torch.zeros(S, H, HD)
        hot[torch.arange(c0, c0 + n), :, torch.arange(n)] = 1.0
        # forward and dK/dV probes
        qkv = torch.cat([torch.zeros(S, 2 * W), hot.view(S, W)], 1).to(DEV).bfloat16()
        out, lse = ops.attn_fwd(qkv, qkv[:, W:], qkv[:, 2 * W:], 3 * W, rows, S, H, SCALE, drop=drop)
        fwd_bits[:, :, c0:c0 + n] = (out.float().view(S, H, HD).permute(1, 0, 2)[..., :n] != 0).cpu()
        d = torch.zeros_like(qkv)
        ops.attn_bwd(qkv, qkv[:, W:], qkv[:, 2 * W:], 3 * W, out, W, lse, hot.view(S, W).to(DEV).bfloat16(), W, d, d[:, W:], d[:, 2 * W:], 3 * W, rows, S, H, SCALE, drop=drop)
        dkv_bits[:, c0:c0 + n, :] = (d[:, 2 * W:].float().view(S, H, HD).permute(1, 2, 0)[:, :n] != 0).cpu()      # [H, d -> query, key]
        # dQ probe
        vv = torch.zeros(S, H, HD)
        vv[:, :, 0] = sign[:, None]
        e0 = torch.zeros(S, H, HD)
        e0[:, :, 0] = 1.0
        qkv = torch.cat([torch.zeros(S, W), hot.view(S, W), vv.view(S, W)], 1).to(DEV).bfloat16()
        out, lse = ops.attn_fwd(qkv, qkv[:, W:], qkv[:, 2 * W:], 3 * W, rows, S, H, SCALE, drop=drop)
        D = out.float().view(S, H, HD)[:, :, 0]      # D_q = dO . O = O[q, 0]
        assert float(D.abs().max()) < 2.0
        d = torch.zeros_like(qkv)
        ops.attn_bwd(qkv, qkv[:, W:], qkv[:, 2 * W:], 3 * W, out, W, lse, e0.view(S, W).to(DEV).bfloat16(), W, d, d[:, W:], d[:, 2 * W:], 3 * W, rows, S, H, SCALE, drop=drop)
        ds = d[:, :W].float().view(S, H, HD) * (S / SCALE) + D[:, :, None]
        dq_bits[:, :, c0:c0 + n] = (ds.abs() > 2.0).permute(1, 0, 2)[..., :n].cpu()
    for name, bits in (("forward", fwd_bits), ("dK/dV kernel", dkv_bits), ("dQ kernel", dq_bits)):
        diff = int((bits != keep).sum())
        print(f"    {name}: {diff} of {keep.numel()} keep bits differ from the counter definition")
        assert diff == 0, name


# ------------------------------------------------------------------------------------------------ 3. continuity with the S <= 256 kernels
def test_continuity_with_the_shipped_kernel_at_256(ops):
    """S = 256 (the shipped kernel) against S = 257 with key 256 masked out and a zero dO on query 256 (csrc/attn_long.hip): the gradients of the first 256 tokens"""
    rows, H = 2, 8
    W = H * HD
    base = rnd(rows, 257, 3 * W, seed=1)
    do = rnd(rows, 257, W, seed=2)
    do[:, 256] = 0
    res = {}
    for S in (256, 257):
        qkv = base[:, :S].reshape(rows * S, 3 * W).to(DEV).bfloat16()
        d_do = do[:, :S].reshape(rows * S, W).to(DEV).bfloat16()
        kvalid = None
        if S == 257:
            kvalid = torch.ones(rows, S, dtype=torch.uint8, device=DEV)
            kvalid[:, 256] = 0
        out, lse = ops.attn_fwd(qkv, qkv[:, W:], qkv[:, 2 * W:], 3 * W, rows, S, H, SCALE, kvalid=kvalid)
        d = torch.zeros_like(qkv)
        ops.attn_bwd(qkv, qkv[:, W:], qkv[:, 2 * W:], 3 * W, out, W, lse, d_do, W, d, d[:, W:], d[:, 2 * W:], 3 * W, rows, S, H, SCALE, kvalid=kvalid)
        res[S] = d.float().view(rows, S, 3 * W)[:, :256].cpu()
    assert bool((res[257].abs().sum() > 0))
    for i, n in enumerate(("dQ", "dK", "dV")):
        a, b = res[257][..., i * W:(i + 1) * W], res[256][..., i * W:(i + 1) * W]
        close(a, b, 2.0 ** -7, 2.0 ** -8 * b.abs().max().item(), f"S=257 (masked key) vs S=256 {n}")


# ------------------------------------------------------------------------------------------------ 4. determinism
def test_two_runs_are_bit_identical(ops):
    rows, S, H = 4, 500, 8
    W = H * HD
    qkv = rnd(rows * S, 3 * W, seed=3).to(DEV).bfloat16()
    d_do = rnd(rows * S, W, seed=4).to(DEV).bfloat16()
    traj = ragged_traj(rows, S, 9).int().to(DEV)
    drop = ops.Dropout(seed=77, stream=2, p=0.1)
    runs = []
    for _ in range(2):
        out, lse = ops.attn_fwd(qkv, qkv[:, W:], qkv[:, 2 * W:], 3 * W, rows, S, H, SCALE, mask_mode=1, traj=traj, drop=drop)
        d = torch.zeros_like(qkv)
        ops.attn_bwd(qkv, qkv[:, W:], qkv[:, 2 * W:], 3 * W, out, W, lse, d_do, W, d, d[:, W:], d[:, 2 * W:], 3 * W, rows, S, H, SCALE, mask_mode=1, traj=traj, drop=drop)
        runs.append(d)
    assert float(runs[0].float().abs().sum()) > 0
    assert torch.equal(runs[0], runs[1])


# ------------------------------------------------------------------------------------------------ 5. what stays refused
def test_s_513_and_bias_above_256_are_refused_and_nothing_is_launched(ops):
    from safevla_amd._lib import SvlaError

    rows, H = 1, 2
    W = H * HD
    for S, with_bias in ((513, False), (300, True)):
        qkv = torch.zeros(rows * S, 3 * W, device=DEV, dtype=torch.bfloat16)
        out = torch.zeros(rows * S, W, device=DEV, dtype=torch.bfloat16)
        lse = torch.zeros(rows, H, S, device=DEV)
        d = torch.full_like(qkv, 7.0)
        bias = torch.zeros(H, S, S, device=DEV) if with_bias else None
        with pytest.raises(SvlaError, match="invalid argument"):
            ops.attn_bwd(qkv, qkv[:, W:], qkv[:, 2 * W:], 3 * W, out, W, lse, out, W, d, d[:, W:], d[:, 2 * W:], 3 * W, rows, S, H, SCALE, bias=bias)
        torch.cuda.synchronize()
        assert bool((d == 7.0).all())


# ------------------------------------------------------------------------------------------------ 6. imitation learning on a whole episode
def test_il_whole_episode_forward_loss_and_gradients_vs_oracle():
    """``small_3``, one trajectory of T = 272 valid steps plus one padded from 120 to 272 (``sliding_window`` = None returns whole trajectories): logits on the valid
    steps, the loss and every parameter gradient against the fp32 CPU oracle (T = 272, not 300: the oracle's forward + backward on the CPU is most of this file's time -- 21 s on
    8 cores at 272, 27 s at 300).  Failed in ``backward()`` (SvlaError) while the attention backward stopped at 256 keys."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from oracle.detfill import fill_state_dict
    from oracle.ref_il import RefEarlyFusion
    from safevla_amd.il import PAD_TOKEN, START_TOKEN, EarlyFusionCnnTransformer

    version = "small_3"
    nf, nd, dd = EarlyFusionCnnTransformer.VERSIONS[version][:3]
    m = EarlyFusionCnnTransformer.build_model(version, device=DEV)
    fill_state_dict(m, seed=9, share_t5=False)
    m.sync_weights()
    m.eval()
    ref = RefEarlyFusion(max_batch=2, n_fusion_layers=nf, n_decoder_layers=nd, dino_dim=dd).eval()
    ref.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()})
    rs = np.random.RandomState(4)
    B, T, L = 2, 272, 6
    valid = np.array([T, 120])
    tt = np.arange(T)[None].repeat(B, 0)
    pad = tt >= valid[:, None]
    actions = rs.randint(0, 20, (B, T))
    last = np.concatenate([np.full((B, 1), START_TOKEN), actions[:, :-1]], 1)
    last[pad], actions[pad] = PAD_TOKEN, -1
    ids = rs.randint(3, 32000, (B, L)); ids[:, -1] = 1
    cpu = {"raw_navigation_camera": torch.from_numpy(rs.standard_normal((B, T, dd, 7, 12)).astype(np.float32)),
           "raw_manipulation_camera": torch.from_numpy(rs.standard_normal((B, T, dd, 7, 12)).astype(np.float32)),
           "time_ids": torch.from_numpy(tt).contiguous(), "an_object_is_in_hand": torch.from_numpy(rs.randint(0, 3, (B, T))),
           "last_actions": torch.from_numpy(last), "actions": torch.from_numpy(actions), "padding_mask": torch.from_numpy(pad),
           "goals": dict(input_ids=torch.from_numpy(ids), attention_mask=torch.ones(B, L, dtype=torch.int64))}
    want = ref(cpu)
    want["loss"].backward()
    batch = {k: (v.to(DEV) if torch.is_tensor(v) else {a: b.to(DEV) for a, b in v.items()}) for k, v in cpu.items()}
    m.zero_grad()
    out = m(batch)
    out["loss"].backward()
    keep = torch.from_numpy(~pad)
    a, b_ = out["actions_logits"].detach().float().cpu()[keep], want["actions_logits"].detach()[keep]
    err = (a - b_).abs().max().item() / (b_.abs().max().item() + 1e-12)
    le = abs(float(out["loss"].detach()) - float(want["loss"])) / abs(float(want["loss"]))
    own = {k.replace("actor.linear.", "actor."): p for k, p in m.named_parameters()}
    errs = []
    for n, p in ref.named_parameters():
        if p.grad is None or float(p.grad.abs().sum()) == 0:
            continue
        errs.append(((own[n].grad.float().cpu() - p.grad).norm() / (p.grad.norm() + 1e-12)).item())
    errs = np.array(errs)
    print(f"    [small_3 B={B} T={T} valid={valid.tolist()}] logits rel-to-max {err:.2e}, loss rel {le:.2e}; parameter-gradient relative L2: median {np.median(errs):.3e} "
          f"max {errs.max():.3e} over {len(errs)}")
    assert err < 3e-2 and le < 3e-2, (err, le)
    assert len(errs) >= 60 and np.median(errs) < 6e-2 and errs.max() < 0.2, (len(errs), np.median(errs), errs.max())


# ------------------------------------------------------------------------------------------------ 7. PPO-Lagrangian over a 320-step rollout
def test_ppo_lagrangian_accumulation_over_a_320_step_rollout_vs_fp32_mode():
    """T = 320, B = 2 (the decoder attends over 320 steps, block-causal on the episodes inside the rollout): one engine accumulation of the three towers (forward, fused
    losses, backward) on the bf16 product path against the fp32 verification mode (svla_attn_bwd_f32 takes S <= 512) on the same weights and rollout.  Raised SvlaError in
    the first decoder backward before."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from safevla_amd.engine import PPOLagConfig, PPOLagEngine
    from safevla_amd.model import SafeDinoLLAMATxNavActorCriticSeparate
    from safevla_amd.synth_env import SynthSpec, fill_synthetic_rollout

    torch.manual_seed(0)
    m16 = SafeDinoLLAMATxNavActorCriticSeparate(device=DEV).eval()
    m32 = SafeDinoLLAMATxNavActorCriticSeparate(device=DEV, precision="fp32").eval()
    m32.load_state_dict(m16.state_dict())
    T, B = 320, 2
    st, nxt, _ = fill_synthetic_rollout(m16, SynthSpec(T=T, B=B, L=12, task="PickUp", seed=21), device=DEV)
    st.compute_returns(nxt["next_value"], nxt["next_c_value"])
    assert float((st.masks[1:T] == 0).sum()) > 0                      # episodes end inside the rollout (block-causal decoder mask matters)
    batch = st.batch_slice(0, B)
    res = {}
    for name, m in (("bf16", m16), ("fp32", m32)):
        eng = PPOLagEngine(m, PPOLagConfig())
        m.zero_grad()
        eng._sums.zero_()
        eng._accumulate(batch, T * B, 0.3)
        res[name] = (m.arena.flat_g.double().clone(), eng._sums.clone())
    (g16, s16), (g32, s32) = res["bf16"], res["fp32"]
    cos = torch.nn.functional.cosine_similarity(g16, g32, dim=0).item()
    rel = ((g16 - g32).norm() / g32.norm()).item()
    print(f"    [fp32 vs bf16 @ T = {T}, B = {B}] loss sums {s16.cpu().numpy()[[0, 1, 2, 4]]} vs {s32.cpu().numpy()[[0, 1, 2, 4]]}; gradient cosine {cos:.6f}, relative L2 error {rel:.3e}")
    np.testing.assert_allclose(s16.cpu().numpy()[[0, 1, 2, 4]], s32.cpu().numpy()[[0, 1, 2, 4]], rtol=1e-2, atol=1e-3 * T * B)
    assert cos > 0.9999 and rel < 1.5e-2, (cos, rel)
    for lo, hi in m16.arena.tower_ranges:
        c = torch.nn.functional.cosine_similarity(g16[lo:hi], g32[lo:hi], dim=0).item()
        assert c > 0.998, c
