"""Last fusion layer with the K / V projections absorbed into its single query (csrc/attn_q1.hip; Tower.absorb_last).

1. the kernel pair and the GEMMs around it against an fp64 restatement of the algebra, next to the materialised path (K / V GEMM + single-query attention + dX GEMM)
   on the same inputs: the absorbed path may be at most 1.5 x as far from fp64 as the materialised one (it rounds qt and c to bf16 where that one rounds K and V)
2. the dropout keep decisions are those of the single-query attention kernel, element for element
3. the whole model on the reference's fixture, absorbed against materialised, eval and train mode
4. deterministic mode stays bitwise repeatable through the new weight-gradient products."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_model_gpu import _three_towers_vs_reference, model, test_train_mode_dropout_vs_oracle as _train_mode_vs_oracle      # noqa: E402,F401  (model: fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
D, H, HD = 512, 8, 64
SCALE = HD ** -0.5
SEED, STREAM = 0x1234ABCD, 8


def _keep(R, S, p):
    """[R, 8, S] float64: keep / (1 - p) of (row, head, query 0, key j), from the oracle's restatement of the counter-based dropout"""
    if p == 0:
        return torch.ones(R, H, S, dtype=torch.float64)
    from oracle.ref_model import hash_dropout

    return hash_dropout(torch.ones(R, H, S, S), SEED, STREAM, p, attn_S=S)[:, :, 0, :].double()


def _inputs(R, S, seed):
    g = torch.Generator().manual_seed(seed)
    bf = lambda t: t.to(torch.bfloat16)
    x = bf(torch.randn(R, S, D, generator=g))
    q0 = bf(torch.randn(R, D, generator=g))
    W = bf(torch.randn(3 * D, D, generator=g) * D ** -0.5)           # k, v of unit scale: scores of order 1, softmax not saturated
    b = torch.randn(3 * D, generator=g) * 0.5
    dao = bf(torch.randn(R, D, generator=g))
    return x, q0, W, b, dao


def _fp64(x, q0, W, b, dao, keep):
    """the algebra of the absorbed form in fp64, on the bf16-rounded operands"""
    x, q0, W, b, dao = (t.double() for t in (x, q0, W, b, dao))
    R = x.shape[0]
    Wk, Wv, bv = W[D:2 * D].view(H, HD, D), W[2 * D:].view(H, HD, D), b[2 * D:].view(H, HD)
    q, do = q0.view(R, H, HD), dao.view(R, H, HD)
    qt = torch.einsum("rhk,hkn->rhn", q, Wk)
    p = torch.softmax(SCALE * torch.einsum("rhn,rjn->rhj", qt, x), -1)
    pd = keep * p
    c, sig = torch.einsum("rhj,rjn->rhn", pd, x), pd.sum(-1)
    o = torch.einsum("rhn,hkn->rhk", c, Wv) + sig[..., None] * bv
    dc, dsig = torch.einsum("rhk,hkn->rhn", do, Wv), (do * bv).sum(-1)
    dp = keep * (torch.einsum("rhn,rjn->rhj", dc, x) + dsig[..., None])
    ds = SCALE * p * (dp - (p * dp).sum(-1, keepdim=True))
    dqt = torch.einsum("rhj,rjn->rhn", ds, x)
    dx = torch.einsum("rhj,rhn->rjn", ds, qt) + torch.einsum("rhj,rhn->rjn", pd, dc)
    dq0 = torch.einsum("rhn,hkn->rhk", dqt, Wk)
    return dict(c=c, sig=sig, o=o.reshape(R, D), dx=dx, dqt=dqt, dq0=dq0.reshape(R, D), pd=pd)


def _absorbed(x, q0, W, b, dao, drop):
    from safevla_amd import ops

    R, S = x.shape[0], x.shape[1]
    x, q0, W, dao, b = (t.to(DEV) for t in (x, q0, W, dao, b))
    Wt = W.t().contiguous()
    eq, _, _ = ops.head_expand(q0, R)
    qt = ops.gemm_nt(eq, Wt[:, D:2 * D], 8 * R, D, D)
    c, sig, P = ops.attn_q1_fwd(x, S * D, qt, R, S, SCALE, drop=drop)
    o = ops.head_pick(ops.gemm_nt(c, W[2 * D:], 8 * R, D, D), R, sigma=sig, bias=b[2 * D:])
    edao, dsig, _ = ops.head_expand(dao, R, bias=b[2 * D:], sigma=sig)
    dc = ops.gemm_nt(edao, Wt[:, 2 * D:], 8 * R, D, D)
    dx, dqt = ops.attn_q1_bwd(x, S * D, qt, dc, dsig, P, R, S, SCALE, drop=drop)
    dq0 = ops.head_pick(ops.gemm_nt(dqt, W[D:2 * D], 8 * R, D, D), R)
    torch.cuda.synchronize()
    return dict(c=c.view(R, H, D), sig=sig, o=o, dx=dx, dqt=dqt.view(R, H, D), dq0=dq0)


def _materialised(x, q0, W, b, dao, drop):
    from safevla_amd import ops

    R, S = x.shape[0], x.shape[1]
    M = R * S
    x, q0, W, dao, b = (t.to(DEV) for t in (x, q0, W, dao, b))
    Wt = W.t().contiguous()
    kv = ops.gemm_nt(x.view(M, D), W[D:], M, 2 * D, D, bias=b[D:])
    ao, lse = ops.attn_fwd(q0, kv, kv[:, D:], 2 * D, R, S, H, SCALE, save_lse=True, Sq=1, ldq=D, drop=drop)
    dq0, dkv = torch.empty(R, D, device=DEV, dtype=torch.bfloat16), torch.empty(M, 2 * D, device=DEV, dtype=torch.bfloat16)
    ops.attn_bwd(q0, kv, kv[:, D:], 2 * D, ao, D, lse, dao, D, dq0, dkv, dkv[:, D:], 2 * D, R, S, H, SCALE, Sq=1, ldq=D, lddq=D, drop=drop)
    dx = ops.gemm_nt(dkv, Wt[:, D:], M, D, 2 * D)
    torch.cuda.synchronize()
    return dict(o=ao, dx=dx.view(R, S, D), dq0=dq0)


def _err(got, want):
    return ((got.double().cpu() - want).abs().max() / want.abs().max()).item()


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("S", [170, 181, 233])
@pytest.mark.parametrize("R", [1, 3])
def test_kernel_pair_vs_fp64_no_further_from_it_than_the_materialised_path(R, S, p):
    """c, sigma, dX, dqt against fp64, each max error relative to the output's largest magnitude held to 1.5 x the materialised path's error on the same inputs.
    That path forms dX, but never c, sigma or dqt: it forms o = W_v c + sigma b_v and dq0 = W_k dqt.  So the kernels' c and sigma are carried through that map in
    fp64 and compared as o (key "c+sig"), dqt likewise as dq0 (key "dqt"): the same quantities on both sides, nothing but the kernels' own outputs on the absorbed
    side.  o and dq0 as the layer really forms them (bf16 pick GEMMs) are held to the same bound.  The direct errors of c and dqt are printed."""
    from safevla_amd import ops

    ins = _inputs(R, S, 100 * R + S)
    want = _fp64(*ins, _keep(R, S, p))
    drop = ops.Dropout(SEED, STREAM, p) if p > 0 else None
    new, old = _absorbed(*ins, drop), _materialised(*ins, drop)
    W, b = ins[2].double(), ins[3].double()
    Wk, Wv, bv = W[D:2 * D].view(H, HD, D), W[2 * D:].view(H, HD, D), b[2 * D:].view(H, HD)
    o_c = torch.einsum("rhn,hkn->rhk", new["c"].double().cpu(), Wv) + new["sig"].double().cpu()[..., None] * bv
    dq0_d = torch.einsum("rhn,hkn->rhk", new["dqt"].double().cpu(), Wk)
    e_new = {"c+sig": _err(o_c.reshape(R, D), want["o"]), "dx": _err(new["dx"], want["dx"]), "dqt": _err(dq0_d.reshape(R, D), want["dq0"]),
             "o": _err(new["o"], want["o"]), "dq0": _err(new["dq0"], want["dq0"])}
    e_old = {k: _err(old[k], want[k]) for k in ("o", "dx", "dq0")}
    direct = {k: _err(new[k], want[k]) for k in ("c", "sig", "dqt")}
    print(f"[R={R} S={S} p={p}] absorbed " + " ".join(f"{k} {v:.3e}" for k, v in e_new.items()) + " | materialised " + " ".join(f"{k} {v:.3e}" for k, v in e_old.items())
          + " | absorbed, direct " + " ".join(f"{k} {v:.3e}" for k, v in direct.items()))
    for k, ref in (("c+sig", "o"), ("dx", "dx"), ("dqt", "dq0"), ("o", "o"), ("dq0", "dq0")):
        assert e_new[k] <= 1.5 * e_old[ref], (k, e_new[k], ref, e_old[ref])


def test_dropout_keep_set_equals_the_single_query_attention_kernels():
    """p = 0.1, S = 181, R = 3.  Probes that expose pd itself: one-hot tokens (x_j = e_j) and qt = 0 make c[r, h, j] = pd[r, h, j] = keep / (1 - p) / S; for the
    materialised kernel K = 0 and V one-hot in (j mod 64) over one 64-key window at a time make o[r, 64 h + d] = pd[r, h, 64 a + d].  Both zero sets equal the oracle's."""
    from safevla_amd import ops

    R, S, p = 3, 181, 0.1
    drop = ops.Dropout(SEED, STREAM, p)
    x = torch.zeros(R, S, D, device=DEV, dtype=torch.bfloat16)
    x[:, torch.arange(S), torch.arange(S)] = 1
    c, sig, P = ops.attn_q1_fwd(x, S * D, torch.zeros(8 * R, D, device=DEV, dtype=torch.bfloat16), R, S, SCALE, drop=drop)
    new_zero = (c.view(R, H, D)[:, :, :S] == 0).cpu()
    q0 = torch.zeros(R, D, device=DEV, dtype=torch.bfloat16)
    old_zero = torch.zeros(R, H, S, dtype=torch.bool)
    for a in range(0, S, HD):
        kv = torch.zeros(R, S, 2 * D, device=DEV, dtype=torch.bfloat16)
        n = min(HD, S - a)
        for h in range(H):
            kv[:, a + torch.arange(n), D + h * HD + torch.arange(n)] = 1
        kv = kv.view(R * S, 2 * D)
        ao, _ = ops.attn_fwd(q0, kv, kv[:, D:], 2 * D, R, S, H, SCALE, save_lse=False, Sq=1, ldq=D, drop=drop)
        old_zero[:, :, a:a + n] = (ao.view(R, H, HD)[:, :, :n] == 0).cpu()
    want_zero = _keep(R, S, p) == 0
    assert 0.05 < want_zero.double().mean().item() < 0.15
    assert torch.equal(new_zero, old_zero) and torch.equal(new_zero, want_zero)
    np.testing.assert_allclose(sig.cpu().numpy(), _keep(R, S, p).sum(-1).numpy() / S, rtol=1e-5)


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_model_gradient_absorbed_vs_materialised_on_the_reference_fixture(model, mode):
    """g5_samelen through the existing fixture checks (eval: the reference's outputs, losses and 252 gradient checksums; train: the oracle with the same dropout
    masks), once per path: both pass those gates, the flat gradients agree, and the absorbed path leaves the K third of the last layer's in_proj_bias.grad exactly 0."""
    from oracle.detfill import grad_probe
    from safevla_amd import ops
    from safevla_amd.losses import SafePPOLogGrad, SafePPOValue

    grads, calls, real = {}, {True: 0, False: 0}, ops.attn_q1_bwd

    def counted(*a, **k):
        calls[absorb] += 1
        return real(*a, **k)

    ops.attn_q1_bwd = counted
    try:
        for absorb in (True, False):
            for t in model.towers:
                t.absorb_last = absorb
            if mode == "eval":
                _three_towers_vs_reference(model, "g5_samelen", True, grad_probe, SafePPOLogGrad, SafePPOValue)
            else:
                _train_mode_vs_oracle(model, True)
            torch.cuda.synchronize()
            grads[absorb] = model.arena.flat_g.double().clone()
            if absorb:
                for t in model.towers:
                    gk = t.visual_encoder.fusion_xformer.layers[-1].self_attn.in_proj_bias.grad[D:2 * D]
                    assert gk.abs().max().item() == 0
    finally:
        ops.attn_q1_bwd = real
        for t in model.towers:
            t.absorb_last = True
        model.zero_grad()
    assert calls == {True: len(model.towers), False: 0}, calls          # the absorbed kernels ran exactly when asked to
    cos = torch.nn.functional.cosine_similarity(grads[True], grads[False], dim=0).item()
    print(f"[{mode}] flat-gradient cosine absorbed vs materialised: {cos:.6f}")
    assert cos > 0.999


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_deterministic_mode_is_bitwise_repeatable_through_the_absorbed_layer(mode):
    """Two updates at T = 4, B = 2 with PPOLagConfig(deterministic=True) from the same parameters (train mode: the same dropout counters): gradients and
    parameters bit-equal, no partial bypassed the fixed-point shadow."""
    from safevla_amd.engine import PPOLagConfig, PPOLagEngine
    from safevla_amd.model import SafeDinoLLAMATxNavActorCriticSeparate
    from safevla_amd.synth_env import SynthSpec, fill_synthetic_rollout

    torch.manual_seed(0)
    m = SafeDinoLLAMATxNavActorCriticSeparate(device=DEV)
    assert all(t.absorb_last for t in m.towers)
    m.train(mode == "train")
    T, B = 4, 2
    st, nxt, ep = fill_synthetic_rollout(m, SynthSpec(T=T, B=B, L=12, task="PickUp", seed=5), device=DEV)
    p0, m0, v0 = m.arena.flat_p.clone(), m.arena.flat_m.clone(), m.arena.flat_v.clone()
    outs = []
    for _ in range(2):
        m.arena.flat_p.copy_(p0); m.arena.flat_m.copy_(m0); m.arena.flat_v.copy_(v0)
        m.sync_weights(frozen=False)
        for t in m.towers:
            t._fwd_count = 0
        eng = PPOLagEngine(m, PPOLagConfig(update_repeats=1, cost_limit=2.31964, deterministic=True, record_small_updates=False))
        info = eng.update(st, nxt["next_value"], nxt["next_c_value"], ep["episode_cost_sum"], ep["n_episodes"])
        torch.cuda.synchronize()
        assert info["det_bypassed_partials"] == 0
        outs.append((m.arena.flat_g.clone(), m.arena.flat_p.clone()))
        del eng
    assert torch.isfinite(outs[0][0]).all() and outs[0][0].abs().sum().item() > 0 and not torch.equal(outs[0][1], p0)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
