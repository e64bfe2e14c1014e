"""``EarlyFusionCnnTransformer(skip_padded_steps=True)``: a batch of trajectories of unequal length (``lengths``) runs everything in front of the decoder on the valid
steps only (il.prepare / Prep.Rf, row_map, row_inv, row_seg; csrc/rows.hip).  ``small_3`` on pre-encoded features, B = 3, T = 8, lengths [8, 5, 1] (Rf = 14 of 24 rows),
goals of two token lengths, eval mode as the gradient tests of tests/test_il_gpu.py run; the fp32 CPU oracle (oracle.ref_il.RefEarlyFusion) on the padded batch is the
reference.  Gradients are taken with the fixed-point accumulation of ``il.deterministic_gradients`` so that "bit for bit" is a property of the code under test and
not of the arrival order of atomics.

Gates (restated from tests/test_il_gpu.py for the 512-wide presets, not loosened): logits on the valid steps relative to the largest < 3e-2; loss within 3e-2 relative;
full-tensor relative L2 error of every parameter gradient: median < 6e-2, max < 0.2, at least 60 tensors."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAV, MANIP = "raw_navigation_camera", "raw_manipulation_camera"
B, T, LENS, RF = 3, 8, (8, 5, 1), 14
GOAL_TOKENS = (6, 4, 6)


def _dev(cpu):
    return {k: (v.to(DEV) if torch.is_tensor(v) else {a: b.to(DEV) for a, b in v.items()}) for k, v in cpu.items()}


def _padded_batch(rs, lens, T, dd=384, cams=(NAV, MANIP), goal_tokens=GOAL_TOKENS):
    """the batch il.Preprocessor builds from samples of these lengths (padding: features 0, actions -1, last_actions 21, in-hand 2, time_ids -1), without ``lengths``"""
    from safevla_amd.il import PAD_TOKEN, START_TOKEN

    nb, L = len(lens), max(goal_tokens)
    tt = np.arange(T)[None].repeat(nb, 0)
    pad = tt >= np.asarray(lens)[:, None]
    actions = rs.randint(0, 20, (nb, T))
    last = np.concatenate([np.full((nb, 1), START_TOKEN), actions[:, :-1]], 1)
    hand = rs.randint(0, 2, (nb, T))
    last[pad], actions[pad], hand[pad], tt[pad] = PAD_TOKEN, -1, 2, -1
    n = np.asarray(goal_tokens[:nb])
    am = (np.arange(L)[None] < n[:, None]).astype(np.int64)
    ids = rs.randint(3, 32000, (nb, L)) * am
    ids[np.arange(nb), n - 1] = 1
    cpu = {"time_ids": torch.from_numpy(tt), "an_object_is_in_hand": torch.from_numpy(hand), "last_actions": torch.from_numpy(last), "actions": torch.from_numpy(actions),
           "padding_mask": torch.from_numpy(pad), "goals": dict(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(am))}
    for c in cams:
        f = rs.standard_normal((nb, T, dd, 7, 12)).astype(np.float32)
        f[pad] = 0.0
        cpu[c] = torch.from_numpy(f)
    return cpu, torch.from_numpy(~pad)


def _grads(m):
    return {k.replace("actor.linear.", "actor."): p.grad.detach().float().cpu().clone() for k, p in m.named_parameters() if p.grad is not None}


def _run(m, batch):
    """forward + backward with bitwise-repeatable accumulation -> dict(logits [B, T, A] fp32 cpu, loss (device scalar), flat (the flat gradient), grads by reference name)"""
    from safevla_amd import ops
    from safevla_amd.il import deterministic_gradients

    nb, nt = batch[m.cameras[0]].shape[:2]
    m.zero_grad()
    ops.det_bypass_count(reset=True)
    with deterministic_gradients(m, nb * nt):
        out = m(batch)
        out["loss"].backward()
    torch.cuda.synchronize()
    assert ops.det_bypass_count(reset=True) == 0          # every partial sum went through the fixed-point shadow: the gradients ARE repeatable
    return dict(logits=out["actions_logits"].detach().float().cpu(), loss=out["loss"].detach().clone(), flat=m.arena.flat_g.clone(), grads=_grads(m))


def _same_bits(a, b, keep=None):
    la, lb = (a["logits"], b["logits"]) if keep is None else (a["logits"][keep], b["logits"][keep])
    return torch.equal(la, lb) and torch.equal(a["loss"], b["loss"]) and torch.equal(a["flat"], b["flat"])


@pytest.fixture(scope="module")
def world():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from oracle.detfill import fill_state_dict
    from oracle.ref_il import RefEarlyFusion
    from safevla_amd.il import EarlyFusionCnnTransformer

    models = {}
    for flag in (False, True):
        m = EarlyFusionCnnTransformer.build_model("small_3", device=DEV, skip_padded_steps=flag)
        fill_state_dict(m, seed=7, share_t5=False)
        m.sync_weights()
        models[flag] = m.eval()
    assert models[True].skip_padded_steps and not models[False].skip_padded_steps
    cpu, keep = _padded_batch(np.random.RandomState(21), LENS, T)
    ref = RefEarlyFusion(max_batch=B).eval()
    ref.load_state_dict({k: v.detach().cpu() for k, v in models[False].state_dict().items()})
    want = ref(cpu)                                          # the reference, once
    want["loss"].backward()
    oracle = dict(logits=want["actions_logits"].detach(), loss=float(want["loss"].detach()),
                  grads={n: p.grad.clone() for n, p in ref.named_parameters() if p.grad is not None and float(p.grad.abs().sum()) > 0})
    base = _dev(cpu)
    lengths = torch.tensor(LENS, dtype=torch.int32)          # a host tensor: read without a device synchronisation
    w = dict(off=models[False], on=models[True], cpu=cpu, keep=keep, oracle=oracle, base=base, lengths=lengths)
    w["run_off"] = _run(models[False], base)                              # today's path: no ``lengths``, no flag
    w["run_on"] = _run(models[True], dict(base, lengths=lengths))         # the skip
    return w


def _distances(a, b, oracle, keep):
    """(logits on the valid steps relative to the oracle's largest, loss relative to the oracle's, {parameter: gradient L2 distance relative to the oracle gradient's norm})"""
    dl = (a["logits"][keep] - b["logits"][keep]).abs().max().item() / (oracle["logits"][keep].abs().max().item() + 1e-12)
    dloss = abs(float(a["loss"]) - float(b["loss"])) / abs(oracle["loss"])
    return dl, dloss, {n: ((a["grads"][n] - b["grads"][n]).norm() / (g.norm() + 1e-12)).item() for n, g in oracle["grads"].items()}


def test_logits_loss_and_gradients_vs_oracle_and_vs_the_padded_path(world):
    keep, oracle = world["keep"], world["oracle"]
    as_run = dict(logits=oracle["logits"], loss=oracle["loss"], grads=oracle["grads"])
    res = {}
    for name in ("run_off", "run_on"):
        dl, dloss, dg = _distances(world[name], as_run, oracle, keep)
        errs = np.array(list(dg.values()))
        print(f"[{name} vs oracle] logits rel-to-max {dl:.3e}, loss rel {dloss:.3e}, gradient rel L2: median {np.median(errs):.3e} max {errs.max():.3e} over {len(errs)}")
        assert dl < 3e-2 and dloss < 3e-2, (name, dl, dloss)
        assert len(errs) >= 60 and np.median(errs) < 6e-2 and errs.max() < 0.2, (name, len(errs), np.median(errs), errs.max())
        assert torch.isfinite(world[name]["logits"]).all() and torch.isfinite(world[name]["flat"]).all()
        res[name] = (dl, dloss, dg)
    # flag on against flag off on the same batch: no further from each other than the padded path is from the oracle, quantity by quantity
    dl, dloss, dg = _distances(world["run_on"], world["run_off"], oracle, keep)
    off_dl, off_dloss, off_dg = res["run_off"]
    worst = max(dg, key=lambda n: dg[n] - off_dg[n])
    print(f"[on vs off] logits {dl:.3e} (off vs oracle {off_dl:.3e}), loss {dloss:.3e} ({off_dloss:.3e}), gradients: max {max(dg.values()):.3e} "
          f"(off vs oracle: min {min(off_dg.values()):.3e}); closest call {worst}: {dg[worst]:.3e} vs {off_dg[worst]:.3e}")
    assert dl <= off_dl and dloss <= off_dloss, (dl, off_dl, dloss, off_dloss)
    assert all(dg[n] <= off_dg[n] for n in dg), [(n, dg[n], off_dg[n]) for n in dg if dg[n] > off_dg[n]]


@pytest.mark.parametrize("attr", ["absorb_last", "prune_last"])
def test_the_other_forms_of_the_last_fusion_layer(world, attr):
    """the last fusion layer as a single query over materialised K / V (absorb_last = False) and as a full layer (prune_last = False; its output gradient then
    returns to compact rows through a strided gather): the same gates against the oracle, and flag on no further from flag off than flag off is from the oracle"""
    keep, oracle = world["keep"], world["oracle"]
    as_run = dict(logits=oracle["logits"], loss=oracle["loss"], grads=oracle["grads"])
    runs = {}
    for name, batch in (("off", world["base"]), ("on", dict(world["base"], lengths=world["lengths"]))):
        m = world[name]
        assert getattr(m, attr) is True
        setattr(m, attr, False)
        try:
            runs[name] = _run(m, batch)
        finally:
            setattr(m, attr, True)
    dist = {name: _distances(runs[name], as_run, oracle, keep) for name in runs}
    for name, (dl, dloss, dg) in dist.items():
        errs = np.array(list(dg.values()))
        print(f"[{attr} = False, {name} vs oracle] logits {dl:.3e}, loss {dloss:.3e}, gradient rel L2: median {np.median(errs):.3e} max {errs.max():.3e}")
        assert dl < 3e-2 and dloss < 3e-2 and len(errs) >= 60 and np.median(errs) < 6e-2 and errs.max() < 0.2, (name, dl, dloss, np.median(errs), errs.max())
    dl, dloss, dg = _distances(runs["on"], runs["off"], oracle, keep)
    print(f"[{attr} = False, on vs off] logits {dl:.3e}, loss {dloss:.3e}, gradients max {max(dg.values()):.3e}")
    assert dl <= dist["off"][0] and dloss <= dist["off"][1] and all(dg[n] <= dist["off"][2][n] for n in dg)
    assert not torch.equal(runs["on"]["flat"], world["run_on"]["flat"])          # (another form did run)


def test_padded_content_cannot_matter(world):
    """NaN features and valid action indices at the padded steps, ``lengths`` on the device: bit for bit the zero-padded, -1 batch; everything finite"""
    keep, cpu = world["keep"], world["cpu"]
    rs = np.random.RandomState(22)
    dirty = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in cpu.items()}
    for c in (NAV, MANIP):
        dirty[c][~keep] = float("nan")
    dirty["actions"][~keep] = torch.from_numpy(rs.randint(0, 20, int((~keep).sum())))
    assert torch.isnan(dirty[NAV]).any() and (dirty["actions"] >= 0).all()
    got = _run(world["on"], dict(_dev(dirty), lengths=world["lengths"].to(DEV)))
    assert torch.isfinite(got["logits"]).all() and torch.isfinite(got["loss"]).all() and torch.isfinite(got["flat"]).all()
    assert got["flat"].abs().sum().item() > 0
    assert _same_bits(got, world["run_on"], keep)


def _arg(decls, call, name):
    fn, args = call
    return args[[n for n, _ in decls[fn.__name__]].index(name)]


def _record(fn):
    from safevla_amd._lib import lib

    L, calls = lib(), []
    assert L.recorder is None
    L.recorder = calls
    try:
        fn()
    finally:
        L.recorder = None
    torch.cuda.synchronize()
    return calls


def test_the_work_really_shrank(world):
    """the row arguments of the compressor GEMMs and of the fusion attention (every form: full, pruned single query, absorbed) are Rf = 14 (x tokens), not 24"""
    from safevla_amd._lib import parse_header

    decls = parse_header()
    S = 1 + 2 * 84 + max(GOAL_TOKENS)
    batch = dict(world["base"], lengths=world["lengths"])
    for name, rows in (("on", RF), ("off", B * T)):
        m = world[name]

        def fwd_bwd():
            m.zero_grad()
            out = m(batch)
            out["loss"].backward()

        def fwd_only():
            with torch.no_grad():
                m(batch)

        for what, calls in (("update", _record(fwd_bwd)), ("no_grad", _record(fwd_only))):
            names = [c[0].__name__ for c in calls]
            comp = [c for c in calls if c[0].__name__ == "svla_gemm_nt_bf16" and _arg(decls, c, "K") == 384 and _arg(decls, c, "N") == 512]
            assert comp and all(_arg(decls, c, "M") == rows * 2 * 84 for c in comp), (name, what, [_arg(decls, c, "M") for c in comp])
            fus = [c for c in calls if c[0].__name__ == "svla_attn_fwd_bf16" and _arg(decls, c, "S") == S]
            q1 = [c for c in calls if c[0].__name__ == "svla_attn_q1_fwd_bf16"]
            assert len(fus) + len(q1) == 3 and (len(q1) == 1 or what == "no_grad"), (name, what, len(fus), len(q1))      # (the update's last layer is the absorbed form)
            assert all(_arg(decls, c, "rows") == rows for c in fus) and all(_arg(decls, c, "R") == rows and _arg(decls, c, "S") == S for c in q1), (name, what)
            assert ("svla_rows_gather" in names) == (name == "on") and ("svla_fusion_text_bwd_seg" in names) == (name == "on" and what == "update"), (name, what)
            # the GEMMs of the full fusion layers (in_proj, out_proj, feed-forward: one row per token)
            fus_rows = [c for c in calls if c[0].__name__ == "svla_gemm_nt_bf16" and _arg(decls, c, "M") in (B * T * S, RF * S)]
            assert fus_rows and all(_arg(decls, c, "M") == rows * S for c in fus_rows), (name, what)


def test_raw_frames_run_the_trunk_on_the_valid_frames_only():
    """B = 2, T = 3, lengths [3, 1], one camera: the frozen trunk sees 4 frames, and the valid steps' logits are those of the padded path (both are the same kernels on
    the same rows: the gate of tests/test_il_gpu.py, relative to the largest logit, is far above what they differ by)"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from oracle.detfill import fill_state_dict
    from safevla_amd._lib import parse_header
    from safevla_amd.il import EarlyFusionCnnTransformer

    decls = parse_header()
    sensors = [NAV, "last_actions", "an_object_is_in_hand"]
    cpu, keep = _padded_batch(np.random.RandomState(23), (3, 1), 3, cams=(), goal_tokens=(5, 3))
    frames = torch.from_numpy(np.random.RandomState(24).randint(0, 256, (2, 3, 224, 384, 3)).astype(np.uint8))
    frames[~keep] = 0
    cpu[NAV] = frames
    batch = dict(_dev(cpu), lengths=torch.tensor([3, 1], dtype=torch.int32))
    logits, trunk = {}, None
    for flag in (False, True):
        m = EarlyFusionCnnTransformer.build_model("small_3", sensors, device=DEV, skip_padded_steps=flag)
        fill_state_dict(m, seed=7, share_t5=False)
        m.sync_weights()
        m.eval()
        m.image_preprocessor = trunk                          # one frozen trunk (its weights are drawn at construction) for both models
        out = {}

        def fwd():
            with torch.no_grad():
                out.update(m(batch))

        calls = _record(fwd)
        trunk = m.image_preprocessor
        seen = [_arg(decls, c, "B") for c in calls if c[0].__name__ == "svla_patchify_u8_bf16"]
        assert seen == [4 if flag else 6], (flag, seen)
        gathers = [c for c in calls if c[0].__name__ == "svla_rows_gather"]
        assert (len(gathers) == 2 and _arg(decls, gathers[0], "row_bytes") == 224 * 384 * 3 and _arg(decls, gathers[0], "rows") == 4) if flag else not gathers
        logits[flag] = out["actions_logits"].float().cpu()
        assert torch.isfinite(logits[flag]).all() and torch.isfinite(out["loss"])
    d = (logits[True][keep] - logits[False][keep]).abs().max().item() / logits[False][keep].abs().max().item()
    print(f"[raw frames] valid-step logits, flag on vs off: rel-to-max {d:.3e}")
    assert d < 3e-2


def test_unchanged_paths_are_bitwise_the_model_without_the_flag(world):
    base, off = world["base"], world["run_off"]
    full = torch.full((B,), T, dtype=torch.int32)
    assert _same_bits(_run(world["on"], dict(base, lengths=full)), off), "flag on, every length = T"
    assert _same_bits(_run(world["on"], dict(base, lengths=full.to(DEV))), off), "flag on, every length = T (device tensor)"
    assert _same_bits(_run(world["on"], base), off), "flag on, no lengths"
    assert _same_bits(_run(world["off"], dict(base, lengths=world["lengths"])), off), "flag off, lengths present"
    assert not torch.equal(world["run_on"]["flat"], off["flat"]) or not torch.equal(world["run_on"]["logits"], off["logits"])      # (the skip itself is another path)


def test_rl_towers_do_not_change_by_a_bit(world):
    """one deterministic update pass and three acting steps of the three RL towers, before and after a ragged IL forward + backward in the same process"""
    from safevla_amd.engine import PPOLagConfig, PPOLagEngine
    from safevla_amd.model import SafeDinoLLAMATxNavActorCriticSeparate
    from safevla_amd.synth_env import SynthSpec, fill_synthetic_rollout

    torch.manual_seed(0)
    m = SafeDinoLLAMATxNavActorCriticSeparate(device=DEV)
    m.eval()
    st, nxt, ep = fill_synthetic_rollout(m, SynthSpec(T=4, B=2, L=12, task="PickUp", seed=5), device=DEV)
    p0, m0, v0 = m.arena.flat_p.clone(), m.arena.flat_m.clone(), m.arena.flat_v.clone()

    def rl_pass():
        m.arena.flat_p.copy_(p0); m.arena.flat_m.copy_(m0); m.arena.flat_v.copy_(v0)
        m.sync_weights(frozen=False)
        for t in m.towers:
            t._fwd_count = 0
        eng = PPOLagEngine(m, PPOLagConfig(update_repeats=1, cost_limit=2.31964, deterministic=True, record_small_updates=False))
        info = eng.update(st, nxt["next_value"], nxt["next_c_value"], ep["episode_cost_sum"], ep["n_episodes"])
        assert info["det_bypassed_partials"] == 0
        outs = [m.arena.flat_g.clone(), m.arena.flat_p.clone()]
        with torch.no_grad():
            for t in range(3):
                o, _ = m({k: v[t:t + 1] for k, v in st.observations.items()}, None, st.prev_actions[t:t + 1], st.masks[t:t + 1])
                outs += [o.distributions.raw_logits.clone(), o.values.clone(), o.c_values.clone()]
        torch.cuda.synchronize()
        return outs

    before = rl_pass()
    ragged = _run(world["on"], dict(world["base"], lengths=world["lengths"]))
    assert _same_bits(ragged, world["run_on"])
    after = rl_pass()
    assert len(before) == len(after) == 11 and all(torch.isfinite(x.float()).all() for x in before) and before[0].abs().sum().item() > 0
    assert all(torch.equal(a, b) for a, b in zip(before, after))


def test_train_mode_steps_repeat_bitwise(world):
    """two ``training_step``s (dropout on: the counters follow the compact row numbering) from the same seed and state: the same parameters, bit for bit; a finite loss"""
    from safevla_amd.il import ILTrainer

    m = world["on"]
    ar = m.arena
    batch = dict(world["base"], lengths=world["lengths"])
    p0, m0, v0 = ar.flat_p.clone(), ar.flat_m.clone(), ar.flat_v.clone()
    outs = []
    try:
        m.train()
        for _ in range(2):
            ar.flat_p.copy_(p0); ar.flat_m.copy_(m0); ar.flat_v.copy_(v0)
            m.sync_weights()
            m._fwd_count = 0
            tr = ILTrainer(m, lr=1e-4, deterministic=True)
            info = tr.training_step(batch)
            torch.cuda.synchronize()
            assert np.isfinite(info["loss"])
            outs.append((ar.flat_p.clone(), ar.flat_g.clone(), info["loss"]))
    finally:
        m.eval()
        ar.flat_p.copy_(p0); ar.flat_m.copy_(m0); ar.flat_v.copy_(v0)
        m.sync_weights()
        m.zero_grad()
    assert not torch.equal(outs[0][0], p0) and torch.isfinite(outs[0][0]).all()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and outs[0][2] == outs[1][2]


def test_validation_counts_the_valid_steps(world):
    """``validation_step`` + ``validation_epoch_end`` on a batch whose padded steps hold valid action indices and NaN features: val_frames = 14, the loss of forward(batch)"""
    from safevla_amd.il import ILTrainer

    keep, m = world["keep"], world["on"]
    dirty = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in world["cpu"].items()}
    dirty["actions"][~keep] = 3
    dirty[NAV][~keep] = float("nan")
    tr = ILTrainer(m)
    tr.validation_step(dict(_dev(dirty), lengths=world["lengths"]))
    out = tr.validation_epoch_end()
    assert out["val_frames"] == RF and not m.training
    assert abs(out["loss/val"] - float(world["run_on"]["loss"])) < 1e-5 * abs(float(world["run_on"]["loss"]))      # the same logits, summed by another kernel (fp32 terms)
    # without the skip the same batch counts every step: the 14 come from the row table, not from the batch's actions
    clean = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in world["cpu"].items()}
    clean["actions"][~keep] = 3
    tr_off = ILTrainer(world["off"])
    tr_off.validation_step(_dev(clean))
    assert tr_off.validation_epoch_end()["val_frames"] == B * T


@pytest.mark.parametrize("lengths,word", [([9, 1, 1], "1 ... 8"), ([0, 1, 1], "1 ... 8"), ([8, 5], "2 entries")])
def test_bad_lengths_are_refused_before_the_first_launch(world, lengths, word):
    batch = dict(world["base"], lengths=torch.tensor(lengths, dtype=torch.int32))

    def fwd():
        with pytest.raises(ValueError, match=word):
            world["on"](batch)

    assert _record(fwd) == []


def test_combinations_that_are_not_carried_through_are_refused_by_name(world):
    m = world["on"]
    batch = dict(world["base"], lengths=world["lengths"])

    def fwd():
        with pytest.raises(ValueError, match="fp8_attention"):
            m(batch)

    m.fp8_attention = True
    try:
        assert _record(fwd) == []
    finally:
        m.fp8_attention = False
    with pytest.raises(TypeError):
        type(m).build_model("small_3", device=DEV, skip_padded=True)


def test_train_il_cli_with_the_flag(tmp_path):
    """``train_il --skip_padded_steps``: the synthetic batches carry ``lengths`` (episodes of random length padded to the window), a few optimiser steps run, losses finite"""
    import json
    import os
    import subprocess
    import sys

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-m", "safevla_amd.train_il", "--per_gpu_batch", "3", "--sliding_window", "7", "--max_samples", "9", "--skip_padded_steps",
                          "--output_dir", str(tmp_path)], cwd=root, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert [l["step"] for l in lines if "loss" in l] == [1, 2, 3] and all(np.isfinite(l["loss"]) for l in lines if "loss" in l)
    assert "timesteps_per_s" in lines[-1]
