"""bf16 MFMA attention for 96-wide heads (csrc/attn_hd96.hip; TransformerConfig(n, 768, 8): ``base_6``, ``siglip_base_3_6``) against an fp64 torch reference,
through the C ABI, through ``ops.attn_fwd`` / ``ops.attn_bwd`` and through ``EarlyFusionCnnTransformer``.

Gates are the 64-wide bf16 kernels' own (tests/test_kernels_gpu.py::_attn_case): output ``close(rtol 1e-2, atol 1e-2)``, gradients
``close(rtol 2e-2, atol 2e-2 * max|want| + 1e-3)``.  Every case prints its worst absolute error (and the gradients' worst error relative to max|want|).

Measured on one MI355X (worst over the cases of each group; every run prints the figures per case):
  no mask S = 5 ... 256, query subsets   O 7.3e-3 abs;  dQ / dK / dV <= 5.7e-3 of max|want|
  block-causal S = 32 / 128 / 256        O 9.9e-3 abs (|want| up to 4.2);  gradients <= 5.6e-3 of max|want|
  kvalid (+ block-causal)                O 8.0e-3 abs;  gradients <= 4.6e-3
  dropout 0.1                            O 1.4e-2 abs (S = 40 block-causal, |want| up to 4.4: inside rtol);  gradients <= 6.1e-3
  fp32 detour, S = 181 with dropout      O 3.5e-3 abs;  gradients <= 2.6e-3 (same seed: the 96-wide MFMA kernels give 3.5e-3 / 4.4e-3)
  base_6 / siglip_base_3_6 padded window vs oracle: logits 1.5e-2 / 1.2e-2 of max, loss 6.1e-4 / 8.4e-4
  base_6 / siglip_base_3_6 train mode vs detour:    logits 1.1e-2 / 1.3e-2, loss 7.1e-4 / 3.3e-5, gradient relative L2 median 3.2e-2 / 2.2e-2, max 6.9e-2 / 5.3e-2
The gradients sit a factor of three inside their gate, as the 64-wide kernels' do; no gate was loosened.  The file takes 11 s on one MI355X, model builds included."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
HD, H, ROWS = 96, 8, 3
SCALE = HD ** -0.5
W = H * HD


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


def hash_mask(seed, stream, p, rows, nq, S):
    """keep-mask [rows, H, nq, S] of the attention-probability dropout: element index ((r*H + h)*S + q) * S4 + k (include/svla.h: svla_dropout)"""
    from oracle.ref_model import hash_keep

    S4 = (S + 3) & ~3
    idx = ((np.arange(rows * H, dtype=np.uint64)[:, None, None] * np.uint64(S) + np.arange(nq, dtype=np.uint64)[None, :, None]) * np.uint64(S4)
           + np.arange(S, dtype=np.uint64)[None, None, :]).reshape(rows, H, nq, S)
    return torch.from_numpy(hash_keep(seed, stream, p, idx))


def ref_attn(q, k, v, mask=None, keep=None, p=0.0):
    """fp64 reference: q [rows, H, nq, 96], k / v [rows, H, S, 96]; mask broadcastable to [rows, H, nq, S] (True = attend)"""
    s = (q @ k.transpose(-1, -2)) * SCALE
    if mask is not None:
        s = s.masked_fill(~mask, float("-inf"))
    pr = torch.softmax(s, -1)
    if keep is not None:
        pr = pr * keep / (1.0 - float(np.float32(p)))
    return pr @ v


def heads(t, n):      # [rows * n, W] -> fp64 leaf [rows, H, n, 96]
    return t.view(ROWS, n, H, HD).transpose(1, 2).double().clone().requires_grad_(True)


def run_case(ops, S, Sq=0, mask_mode=0, traj=None, kvalid=None, p=0.0, seed=0, name=""):
    """one forward + backward at head_dim 96 through ops.attn_fwd / ops.attn_bwd against the fp64 reference"""
    attn_fwd, attn_bwd = ops.attn_fwd, ops.attn_bwd
    nq = Sq or S
    kv, qs = rnd(ROWS * S, 2 * W, seed=seed + 1), rnd(ROWS * nq, W, seed=seed + 2)
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
        keep = hash_mask(0xBEEF, 4, p, ROWS, nq, S)
    want = ref_attn(q, k, v, mask, keep, p)
    kw = dict(mask_mode=mask_mode, traj=None if traj is None else traj.int().to(DEV), kvalid=None if kvalid is None else kvalid.to(torch.uint8).to(DEV),
              drop=drop, head_dim=HD)
    d_kv, d_q = kv.to(DEV).bfloat16(), qs.to(DEV).bfloat16()
    if Sq:
        out, lse = attn_fwd(d_q, d_kv, d_kv[:, W:], 2 * W, ROWS, S, H, SCALE, Sq=Sq, ldq=W, **kw)
    else:      # all queries: q laid out like k / v (one fused tensor)
        qkv = torch.cat([d_q, d_kv], 1)
        out, lse = attn_fwd(qkv, qkv[:, W:], qkv[:, 2 * W:], 3 * W, ROWS, S, H, SCALE, **kw)
    assert out.dtype == torch.bfloat16 and out.shape == (ROWS * nq, W) and lse.shape == (ROWS, H, nq)
    close(out.float().view(ROWS, nq, H, HD), want.transpose(1, 2), 1e-2, 1e-2, f"{name} O")
    do = rnd(ROWS * nq, W, seed=seed + 5)
    want.backward(do.view(ROWS, nq, H, HD).transpose(1, 2).double())
    d_do = do.to(DEV).bfloat16()
    if Sq:
        dq, dkv = torch.zeros_like(d_q), torch.zeros_like(d_kv)
        attn_bwd(d_q, d_kv, d_kv[:, W:], 2 * W, out, W, lse, d_do, W, dq, dkv, dkv[:, W:], 2 * W, ROWS, S, H, SCALE, Sq=Sq, ldq=W, lddq=W, **kw)
        got = [dq.view(ROWS, nq, H, HD), dkv[:, :W].view(ROWS, S, H, HD), dkv[:, W:].view(ROWS, S, H, HD)]
    else:
        dqkv = torch.zeros_like(qkv)
        attn_bwd(qkv, qkv[:, W:], qkv[:, 2 * W:], 3 * W, out, W, lse, d_do, W, dqkv, dqkv[:, W:], dqkv[:, 2 * W:], 3 * W, ROWS, S, H, SCALE, **kw)
        got = [dqkv[:, i * W:(i + 1) * W].view(ROWS, S, H, HD) for i in range(3)]
    for g_, t, n in zip(got, (q, k, v), ("dQ", "dK", "dV")):
        w = t.grad.transpose(1, 2)
        close(g_.float(), w, 2e-2, 2e-2 * w.abs().max().item() + 1e-3, f"{name} {n}")


# ------------------------------------------------------------------------------------------------ 1. the C ABI
def test_c_abi_accepts_head_dim_96_and_refuses_what_it_does_not_cover(ops):
    """svla_attn_fwd_bf16 / svla_attn_bwd_bf16 called directly with head_dim = 96 (SVLA_EINVAL before the 96-wide kernels existed); S = 300 and the T5 bias stay refused."""
    from safevla_amd._lib import SvlaError, lib

    S = 100
    qkv = rnd(ROWS * S, 3 * W, seed=1)
    q, k, v = heads(qkv[:, :W], S), heads(qkv[:, W:2 * W], S), heads(qkv[:, 2 * W:], S)
    want = ref_attn(q, k, v)
    d = qkv.to(DEV).bfloat16()
    out = torch.zeros(ROWS * S, W, device=DEV, dtype=torch.bfloat16)
    lse = torch.zeros(ROWS, H, S, device=DEV)
    p_, st = ops._p, ops._stream()
    lib().call("svla_attn_fwd_bf16", p_(d), p_(d[:, W:]), p_(d[:, 2 * W:]), 3 * W, p_(out), W, p_(lse), ROWS, S, H, 96, float(SCALE), 0, None, None, None, 0, 0, 0, None, st)
    close(out.float().view(ROWS, S, H, HD), want.transpose(1, 2), 1e-2, 1e-2, "C ABI O")
    s = (q @ k.transpose(-1, -2)) * SCALE
    close(lse, torch.logsumexp(s, -1), 1e-3, 1e-3, "C ABI LSE")
    do = rnd(ROWS * S, W, seed=2)
    want.backward(do.view(ROWS, S, H, HD).transpose(1, 2).double())
    dd = torch.zeros_like(d)
    d_do = do.to(DEV).bfloat16()
    for d_ws in (None, torch.zeros(ROWS * H * S, device=DEV)):      # both forms of the D = rowsum(dO * O) hand-over
        dd.zero_()
        lib().call("svla_attn_bwd_bf16", p_(d), p_(d[:, W:]), p_(d[:, 2 * W:]), 3 * W, p_(out), W, p_(lse), p_(d_do), W, p_(dd), p_(dd[:, W:]), p_(dd[:, 2 * W:]), 3 * W,
                   ROWS, S, H, 96, float(SCALE), 0, None, None, None, 0, 0, 0, p_(d_ws), None, st)
        for i, (n, t) in enumerate((("dQ", q), ("dK", k), ("dV", v))):
            w = t.grad.transpose(1, 2)
            close(dd[:, i * W:(i + 1) * W].float().view(ROWS, S, H, HD), w, 2e-2, 2e-2 * w.abs().max().item() + 1e-3, f"C ABI {n} (D_ws {'given' if d_ws is not None else 'null'})")
    # unsupported at 96: refused, nothing launched (the output buffer keeps its sentinel)
    S2 = 300
    big = torch.zeros(ROWS * S2, 3 * W, device=DEV, dtype=torch.bfloat16)
    out2 = torch.full((ROWS * S2, W), 7.0, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(SvlaError, match="invalid argument"):
        lib().call("svla_attn_fwd_bf16", p_(big), p_(big[:, W:]), p_(big[:, 2 * W:]), 3 * W, p_(out2), W, None, ROWS, S2, H, 96, float(SCALE), 0, None, None, None, 0, 0, 0, None, st)
    bias = torch.zeros(H, S, S, device=DEV)
    out3 = torch.full((ROWS * S, W), 7.0, device=DEV, dtype=torch.bfloat16)
    with pytest.raises(SvlaError, match="invalid argument"):
        lib().call("svla_attn_fwd_bf16", p_(d), p_(d[:, W:]), p_(d[:, 2 * W:]), 3 * W, p_(out3), W, None, ROWS, S, H, 96, float(SCALE), 0, None, p_(bias), None, 0, 0, 0, None, st)
    with pytest.raises(SvlaError, match="invalid argument"):
        lib().call("svla_attn_bwd_bf16", p_(d), p_(d[:, W:]), p_(d[:, 2 * W:]), 3 * W, p_(out), W, p_(lse), p_(d_do), W, p_(dd), p_(dd[:, W:]), p_(dd[:, 2 * W:]), 3 * W,
                   ROWS, S, H, 96, float(SCALE), 0, None, p_(bias), None, 0, 0, 0, None, None, st)
    with pytest.raises(SvlaError, match="invalid argument"):      # any other width
        lib().call("svla_attn_fwd_bf16", p_(d), p_(d[:, W:]), p_(d[:, 2 * W:]), 3 * W, p_(out3), W, None, ROWS, S, H, 80, float(SCALE), 0, None, None, None, 0, 0, 0, None, st)
    torch.cuda.synchronize()
    assert bool((out2 == 7.0).all()) and bool((out3 == 7.0).all())


# ------------------------------------------------------------------------------------------------ 2. parity over the mode table
@pytest.mark.parametrize("S", [5, 16, 64, 100, 181, 192, 233, 256])
def test_nomask(ops, S):
    run_case(ops, S, name=f"S={S}")


@pytest.mark.parametrize("Sq", [1, 5, 20])
def test_query_subset(ops, Sq):
    """Sq > 0: only the first Sq queries of every row (the pruned last fusion layer: Sq = 1)"""
    run_case(ops, 181, Sq=Sq, name=f"S=181 Sq={Sq}")


@pytest.mark.parametrize("S", [32, 128, 256])
def test_block_causal(ops, S):
    g = torch.Generator().manual_seed(S)
    traj = torch.cumsum((torch.rand(ROWS, S, generator=g) < 0.05).long(), dim=1) + 3      # random trajectory boundaries inside the window
    run_case(ops, S, mask_mode=1, traj=traj, name=f"block-causal S={S}")


def test_kvalid_ragged(ops):
    S = 77
    kvalid = torch.zeros(ROWS, S)
    for i, n in enumerate([77, 30, 1]):      # a full row, a ragged one, a row with a single valid key
        kvalid[i, :n] = 1
    run_case(ops, S, kvalid=kvalid, name="kvalid S=77")
    S = 200                                  # with the block-causal mask on top (decoder over a padded window)
    kvalid = torch.ones(ROWS, S)
    kvalid[1, 150:] = 0
    kvalid[2, 1:] = 0
    run_case(ops, S, mask_mode=1, traj=torch.zeros(ROWS, S, dtype=torch.long), kvalid=kvalid, name="kvalid + causal S=200")


@pytest.mark.parametrize("S,causal", [(40, True), (100, False), (181, False)])
def test_dropout(ops, S, causal):
    traj = torch.sort(torch.randint(0, 3, (ROWS, S), generator=torch.Generator().manual_seed(3)), dim=1).values if causal else None
    run_case(ops, S, mask_mode=int(causal), traj=traj, p=0.1, name=f"dropout S={S}{' block-causal' if causal else ''}")
    if S == 181:
        run_case(ops, S, Sq=1, p=0.1, name="dropout S=181 Sq=1")      # the pruned last fusion layer in train mode


@pytest.mark.parametrize("save_lse", [True, False])
def test_kv_rows_single_query(ops, save_lse):
    """kv_rows > S (K / V sit in a cache of kv_rows token rows per batch row), Sq = 1, forward only"""
    S, kvr = 50, 64
    cache, qs = rnd(ROWS * kvr, 2 * W, seed=1), rnd(ROWS, W, seed=2)
    used = cache.view(ROWS, kvr, 2 * W)[:, :S].reshape(ROWS * S, 2 * W)
    want = ref_attn(heads(qs, 1), heads(used[:, :W].contiguous(), S), heads(used[:, W:].contiguous(), S))
    d_c = cache.to(DEV).bfloat16()
    out, lse = ops.attn_fwd(qs.to(DEV).bfloat16(), d_c, d_c[:, W:], 2 * W, ROWS, S, H, SCALE, Sq=1, ldq=W, kv_rows=kvr, save_lse=save_lse, head_dim=HD)
    assert (lse is not None) == save_lse
    close(out.float().view(ROWS, 1, H, HD), want.transpose(1, 2), 1e-2, 1e-2, f"kv_rows={kvr} S={S} Sq=1 save_lse={save_lse}")


# ------------------------------------------------------------------------------------------------ 3. dropout masks, exactly
def test_dropout_masks_bit_equal_hash_keep(ops):
    """V = the first S columns of an identity (padded to 96): O is the dropped probability row itself, so its zero pattern is the keep-mask"""
    S, p = 77, 0.1
    qk = rnd(ROWS * S, 2 * W, seed=11)
    v = torch.zeros(ROWS, S, H, HD)
    v[:, torch.arange(S), :, torch.arange(S)] = 1.0
    qkv = torch.cat([qk, v.view(ROWS * S, W)], 1).to(DEV).bfloat16()
    out, _ = ops.attn_fwd(qkv, qkv[:, W:], qkv[:, 2 * W:], 3 * W, ROWS, S, H, SCALE, drop=ops.Dropout(seed=0xBEEF, stream=4, p=p), head_dim=HD)
    got = out.float().view(ROWS, S, H, HD).permute(0, 2, 1, 3)[..., :S].cpu() != 0      # [rows, H, q, k]
    keep = hash_mask(0xBEEF, 4, p, ROWS, S, S).bool()
    assert got.shape == keep.shape and bool((got == keep).all()), int((got != keep).sum())
    assert 0.05 < 1.0 - keep.float().mean().item() < 0.15


# ------------------------------------------------------------------------------------------------ 4. routing
def test_ops_route_has_no_fp32_copies_and_the_switch_restores_the_detour(ops, monkeypatch):
    S = 181
    qkv = rnd(ROWS * S, 3 * W, seed=21).to(DEV).bfloat16()
    one_fp32_copy = ROWS * S * W * 4

    def growth():
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        o, l = ops.attn_fwd(qkv, qkv[:, W:], qkv[:, 2 * W:], 3 * W, ROWS, S, H, SCALE, head_dim=HD)
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, o

    monkeypatch.delenv("SVLA_ATTN96_F32", raising=False)
    g_new, o_new = growth()
    monkeypatch.setenv("SVLA_ATTN96_F32", "1")
    g_old, o_old = growth()
    print(f"    peak allocation growth over ops.attn_fwd: MFMA route {g_new} B, fp32 detour {g_old} B (one fp32 copy of Q = {one_fp32_copy} B)")
    assert g_new < one_fp32_copy <= g_old
    close(o_new.float(), o_old.float(), 1e-2, 1e-2, "route vs detour O")
    # the detour against the same fp64 reference and gates, forward and backward (it is the A/B baseline of tools/ab_attn96.py)
    run_case(ops, S, p=0.1, name="detour S=181 dropout")
    monkeypatch.delenv("SVLA_ATTN96_F32")
    # S > 256 stays on the detour whatever the switch says
    S2 = 300
    big = rnd(ROWS * S2, 3 * W, seed=22).to(DEV).bfloat16()
    o2, _ = ops.attn_fwd(big, big[:, W:], big[:, 2 * W:], 3 * W, ROWS, S2, H, SCALE, head_dim=HD)
    assert bool(torch.isfinite(o2.float()).all())


# ------------------------------------------------------------------------------------------------ 5. the two presets
_MODELS = {}


def _model(version):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    if version not in _MODELS:
        from oracle.detfill import fill_state_dict
        from safevla_amd.il import EarlyFusionCnnTransformer

        m = EarlyFusionCnnTransformer.build_model(version, device=DEV)
        fill_state_dict(m, seed=13, share_t5=False)
        m.sync_weights()
        m.eval()
        _MODELS[version] = m
    return _MODELS[version]


def _window_batch(version, B, T, seed, padded):
    from safevla_amd.il import PAD_TOKEN, START_TOKEN, EarlyFusionCnnTransformer

    _, _, dd, te, _, _, _ = EarlyFusionCnnTransformer.version_config(version)
    rs = np.random.RandomState(seed)
    valid = rs.randint(1, T + 1, B) if padded else np.full(B, T)
    valid[rs.randint(0, B)] = T                                  # at least one full-length trajectory
    tt = np.arange(T)[None].repeat(B, 0)
    pad = tt >= valid[:, None]
    actions = rs.randint(0, 20, (B, T))
    last = np.concatenate([np.full((B, 1), START_TOKEN), actions[:, :-1]], 1)
    last[pad], actions[pad] = PAD_TOKEN, -1
    if te == "t5-small":
        L = 9
        n = rs.randint(2, L + 1, B); n[0] = L
        ids = rs.randint(3, 32000, (B, L))
        am = (np.arange(L)[None] < n[:, None]).astype(np.int64)
        ids = ids * am
        ids[np.arange(B), n - 1] = 1
        goals = dict(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(am))
    else:
        ids = np.ones((B, 64), np.int64)
        for b in range(B):
            k = rs.randint(3, 20)
            ids[b, :k] = rs.randint(3, 32000, k)
        goals = torch.from_numpy(ids)
    cpu = {"raw_navigation_camera": torch.from_numpy(rs.standard_normal((B, T, dd, 7, 12)).astype(np.float32)),
           "raw_manipulation_camera": torch.from_numpy(rs.standard_normal((B, T, dd, 7, 12)).astype(np.float32)),
           "time_ids": torch.from_numpy(tt).contiguous(), "an_object_is_in_hand": torch.from_numpy(rs.randint(0, 3, (B, T))),
           "last_actions": torch.from_numpy(last), "actions": torch.from_numpy(actions), "padding_mask": torch.from_numpy(pad), "goals": goals}
    dev = {k: (v.to(DEV) if torch.is_tensor(v) else {a: b_.to(DEV) for a, b_ in v.items()}) for k, v in cpu.items()}
    return cpu, dev, pad, valid


@pytest.mark.parametrize("version", ["base_6", "siglip_base_3_6"])
def test_preset_padded_window_vs_oracle(version):
    """B = 3 trajectories of a T = 13 window padded from ragged lengths, eval mode, against the fp32 oracle restatement: logits on the valid steps and the loss
    within 3e-2 relative (the gate of tests/test_il_gpu.py::test_random_window_shapes_with_padding_vs_oracle)"""
    from oracle.ref_il import RefEarlyFusion
    from safevla_amd.il import EarlyFusionCnnTransformer

    m = _model(version)
    nf, nd, dd, te, dm, nh, nhd = EarlyFusionCnnTransformer.version_config(version)
    assert m.hdim == 96 and m.adt == torch.bfloat16
    B, T = 3, 13
    ref = RefEarlyFusion(max_batch=B, n_fusion_layers=nf, n_decoder_layers=nd, dino_dim=dd, text_encoder=te, d_model=dm, n_heads=nh, n_heads_decoder=nhd).eval()
    ref.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()})
    cpu, dev, pad, valid = _window_batch(version, B, T, seed=105, padded=True)
    with torch.no_grad():
        want = ref(cpu)
        out = m(dev)
    keep = torch.from_numpy(~pad)
    a, b_ = out["actions_logits"].detach().float().cpu()[keep], want["actions_logits"].detach()[keep]
    err = (a - b_).abs().max().item() / (b_.abs().max().item() + 1e-12)
    le = abs(float(out["loss"]) - float(want["loss"])) / abs(float(want["loss"]))
    print(f"    [{version} B={B} T={T} valid={valid.tolist()}] logits rel-to-max {err:.2e}, loss rel {le:.2e}")
    assert err < 3e-2 and le < 3e-2, (err, le)


@pytest.mark.parametrize("version", ["base_6", "siglip_base_3_6"])
def test_preset_train_mode_new_route_vs_fp32_detour(version, monkeypatch):
    """train mode (dropout active, ``drop_seed_base`` and the pass counter fixed): the MFMA route against the fp32 detour of the SAME model with the same dropout
    counters.  Logits / loss within 3e-2 relative; parameter-gradient relative L2 errors gated at the figures tests/test_il_gpu.py uses for 768-wide models."""
    m = _model(version)
    _, dev, pad, _ = _window_batch(version, 3, 13, seed=106, padded=True)

    def one_pass():
        m.train()
        try:
            m.drop_seed_base, m._fwd_count = 4242, 0
            m.zero_grad()
            out = m(dev)
            out["loss"].backward()
            torch.cuda.synchronize()
            grads = {n: p.grad.detach().float().cpu().clone() for n, p in m.named_parameters() if p.grad is not None}
            return out["actions_logits"].detach().float().cpu().clone(), float(out["loss"].detach()), grads
        finally:
            m.eval()

    monkeypatch.delenv("SVLA_ATTN96_F32", raising=False)
    lg_new, loss_new, g_new = one_pass()
    monkeypatch.setenv("SVLA_ATTN96_F32", "1")
    lg_old, loss_old, g_old = one_pass()
    keep = torch.from_numpy(~pad)
    err = (lg_new[keep] - lg_old[keep]).abs().max().item() / (lg_old[keep].abs().max().item() + 1e-12)
    le = abs(loss_new - loss_old) / abs(loss_old)
    errs = np.array([((g_new[n] - g).norm() / (g.norm() + 1e-12)).item() for n, g in g_old.items()
                     if float(g.abs().sum()) != 0 and "text_encoder" not in n and not n.startswith("critic.")])
    print(f"    [{version} train] logits rel-to-max {err:.2e}, loss rel {le:.2e}; parameter-gradient relative L2: median {np.median(errs):.3e} max {errs.max():.3e} over {len(errs)}")
    assert err < 3e-2 and le < 3e-2, (err, le)
    assert len(errs) >= 60 and np.median(errs) < 0.12 and errs.max() < 0.35, (len(errs), np.median(errs), errs.max())
