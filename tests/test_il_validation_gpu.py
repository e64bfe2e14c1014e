"""ILTrainer.validation_step / validation_epoch_end (il.py; LitModel.validation_step / on_validation_epoch_end of training/offline/train_pl.py:187-281) and the
``--eval_every`` loop of train_il.py.

The reference of (a), (d), (e) is the model's OWN eval-mode ``forward(batch)["actions_logits"]`` pushed through torch.argmax, the numpy restatement of the kernel
contract and of the F1 arithmetic (tests/helpers/action_metrics_ref.py) and an fp64 cross-entropy: the forward is pinned elsewhere (tests/test_il_gpu.py), what is
checked here is everything between the logits and the log keys -- row order, padding, accumulation over batches, the epoch's reset.  Gates: F1 keys 1e-12, the
confusion matrix exact, the loss within 2e-6 * max(1, |want|) on the summed cross-entropy (tests/test_kernels_gpu.py::test_ce_loss_fwd_bwd_vs_torch)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import action_metrics_ref as R      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_MODELS = {}


def _trainer():
    """one small_3 model (all four sensors) with fill_state_dict weights and its trainer, for the whole module"""
    if "tr" not in _MODELS:
        from oracle.detfill import fill_state_dict
        from safevla_amd.il import EarlyFusionCnnTransformer, ILTrainer

        m = EarlyFusionCnnTransformer.build_model("small_3", device=DEV)
        fill_state_dict(m, seed=21, share_t5=False)
        m.sync_weights()
        _MODELS["tr"] = ILTrainer(m.eval())
    return _MODELS["tr"]


def _batch(seed, B, T, valid):
    """A padded batch of pre-encoded features: features, goal table and in-hand values as train_il.synthetic_batch draws them, the padding planted: trajectory b
    has valid[b] steps, the rest is padded as the dataset pads (actions = -1, last_actions = 21)"""
    from safevla_amd.il import PAD_TOKEN, START_TOKEN
    from safevla_amd.train_il import synthetic_batch

    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    batch = synthetic_batch(B, T, 6, DEV, g)
    pad = torch.arange(T, device=DEV)[None, :] >= torch.tensor(valid, device=DEV)[:, None]
    actions = torch.randint(0, 20, (B, T), device=DEV, generator=g)
    last = torch.cat([torch.full((B, 1), START_TOKEN, device=DEV), actions[:, :-1]], 1)
    batch.update(padding_mask=pad, actions=torch.where(pad, torch.full_like(actions, -1), actions), last_actions=torch.where(pad, torch.full_like(last, PAD_TOKEN), last))
    return batch


def _agree(model, batch):
    """Every second valid step's target becomes the model's own greedy action there, so that the confusion matrix has a diagonal and the F1 keys are not all 0
    (last_actions stays as it is: the logits do not move)"""
    with torch.no_grad():
        pred = model(batch)["actions_logits"].argmax(-1)
    T = pred.shape[1]
    take = (torch.arange(T, device=DEV)[None, :] % 2 == 0) & ~batch["padding_mask"]
    batch["actions"] = torch.where(take, pred, batch["actions"])
    return batch


def _reference(model, batches):
    """(confusion [20, 20], summed fp64 cross-entropy, frames) of the model's own eval-mode forward over ``batches``"""
    C, loss, frames = np.zeros((20, 20), np.int64), 0.0, 0
    assert not model.training
    for b in batches:
        with torch.no_grad():
            logits = model(b)["actions_logits"]                   # [B, T, 20]
        x, t = logits.reshape(-1, 20).double().cpu(), b["actions"].reshape(-1).cpu()
        keep = t != -1
        pred = torch.argmax(logits.reshape(-1, 20), -1).cpu()
        np.add.at(C, (t[keep].numpy(), pred[keep].numpy()), 1)
        loss += float(torch.nn.functional.cross_entropy(x[keep], t[keep], reduction="sum"))
        frames += int(keep.sum())
        c2, s2, p2 = R.metrics(x.numpy(), t.numpy())              # the helper says the same as torch
        assert np.array_equal(p2, pred.numpy()) and s2[1] == int(keep.sum()) and s2[2] == 0
    return C, loss, frames


def _check_epoch(val, C, loss, frames, confusion=None):
    from safevla_amd.agent import ALL_STRETCH_ACTIONS

    per, macro, weighted = R.f1(C)
    assert len(val) == 25 and val["val_frames"] == frames
    assert abs(val["f1score_macro/val"] - macro) <= 1e-12 and abs(val["f1score_weighted/val"] - weighted) <= 1e-12
    for k, name in enumerate(ALL_STRETCH_ACTIONS):
        assert abs(val[f"f1score/{name}/val"] - per[k]) <= 1e-12, name
    err, gate = abs(val["actions_loss/val"] * frames - loss), 2e-6 * max(1.0, abs(loss))
    print(f"summed loss {val['actions_loss/val'] * frames:.9f}, fp64 {loss:.9f}: |diff| {err:.3e}, gate {gate:.3e}; frames {frames}; macro F1 {macro:.6f}")
    assert err <= gate and val["loss/val"] == val["actions_loss/val"]
    if confusion is not None:
        assert confusion.dtype == np.int64 and np.array_equal(confusion, C)


def test_a_two_batches_against_the_models_own_forward_and_e_the_next_epoch_starts_from_zero():
    tr = _trainer()
    batches = [_agree(tr.model, _batch(1, 3, 8, [8, 5, 3])), _agree(tr.model, _batch(2, 3, 8, [4, 8, 6]))]
    C, loss, frames = _reference(tr.model, batches)
    assert frames == 16 + 18 and C.sum() == frames and np.trace(C) >= 10 and R.f1(C)[1] > 0
    for b in batches:
        assert tr.validation_step(b) is None
    confusion = tr.val_metrics.counts.cpu().numpy()
    _check_epoch(tr.validation_epoch_end(), C, loss, frames, confusion)
    # (e) a second epoch, on the second batch alone: nothing of the first epoch is left
    assert int(tr.val_metrics.counts.abs().sum()) == 0 and tr.val_metrics.sums.tolist() == [0.0, 0.0, 0.0]
    C2, loss2, frames2 = _reference(tr.model, batches[1:])
    tr.validation_step(batches[1])
    confusion = tr.val_metrics.counts.cpu().numpy()
    _check_epoch(tr.validation_epoch_end(), C2, loss2, frames2, confusion)


def test_b_one_step_is_one_metrics_launch_without_the_loss_kernel_or_a_backward():
    from safevla_amd._lib import lib

    tr = _trainer()
    b = _batch(3, 3, 8, [8, 5, 3])
    L = lib()
    assert L.recorder is None
    calls = L.recorder = []
    try:
        tr.validation_step(b)
    finally:
        L.recorder = None
    names = [fn.__name__ for fn, _ in calls]
    tr.val_metrics.reset()
    assert names.count("svla_action_metrics_f32") == 1 and names[-1] == "svla_action_metrics_f32"
    assert "svla_ce_loss_fwd_bwd_f32" not in names
    assert not [n for n in names if "bwd" in n or "adam" in n], names
    assert len(names) > 10                                        # the tower forward itself was recorded


@pytest.mark.parametrize("training", [False, True])
def test_c_weights_optimiser_state_and_mode_are_untouched(training):
    tr = _trainer()
    m, ar = tr.model, tr.model.arena
    before = [t.clone() for t in (ar.flat_p, ar.flat_m, ar.flat_v)]
    steps = tr.step_count
    m.train(training)
    try:
        tr.validation_step(_batch(4, 3, 8, [8, 5, 3]))
        assert m.training is training
        val = tr.validation_epoch_end()
        assert m.training is training and all(mod.training is training for mod in m.modules())
    finally:
        m.eval()
    assert val["val_frames"] == 16 and tr.step_count == steps
    for a, b in zip(before, (ar.flat_p, ar.flat_m, ar.flat_v)):
        assert torch.equal(a, b)


def test_d_a_window_of_513_steps_validates():
    tr = _trainer()
    b = _agree(tr.model, _batch(5, 1, 513, [500]))
    C, loss, frames = _reference(tr.model, [b])
    assert frames == 500 and np.trace(C) >= 250
    tr.validation_step(b)
    confusion = tr.val_metrics.counts.cpu().numpy()
    _check_epoch(tr.validation_epoch_end(), C, loss, frames, confusion)


def test_compute_refuses_an_epoch_with_nan_logits():
    """A diverged model reports no F1: NaN logits into the epoch's state -> validation_epoch_end raises, and the next epoch starts from zero"""
    tr = _trainer()
    logits = torch.zeros(4, 20, device=DEV)
    logits[2, 5] = float("nan")
    tr.val_metrics.update(logits, torch.tensor([1, 2, 3, -1], device=DEV))
    with pytest.raises(ValueError, match="1 rows"):
        tr.validation_epoch_end()
    assert int(tr.val_metrics.counts.abs().sum()) == 0 and tr.val_metrics.sums.tolist() == [0.0, 0.0, 0.0]


def test_f_train_il_eval_every():
    from safevla_amd.agent import ALL_STRETCH_ACTIONS

    keys = {"f1score_weighted/val", "f1score_macro/val", "actions_loss/val", "loss/val", "val_frames"} | {f"f1score/{n}/val" for n in ALL_STRETCH_ACTIONS}
    assert len(keys) == 25
    cmd = ["timeout", "-k", "10", "600", sys.executable, "-m", "safevla_amd.train_il", "--max_samples", "64", "--per_gpu_batch", "4", "--sliding_window", "8"]
    out = subprocess.run(cmd + ["--eval_every", "2", "--eval_max_samples", "8"], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    vals = [l for l in lines if "val" in l]
    assert [l["step"] for l in vals] == list(range(2, 17, 2)), out.stdout
    for l in vals:
        assert set(l["val"]) == keys and all(math.isfinite(v) for v in l["val"].values()), l
        assert 8 <= l["val"]["val_frames"] <= 2 * 4 * 8 and 0.0 <= l["val"]["f1score_macro/val"] <= 1.0 and l["val"]["loss/val"] > 0
    assert len({l["val"]["val_frames"] for l in vals}) == 1       # the same held-out batches at every validation
    assert any("timesteps_per_s" in l for l in lines)
    off = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    assert off.returncode == 0, off.stderr[-2000:]
    assert '"val"' not in off.stdout and '"timesteps_per_s"' in off.stdout
    # the training lines are printed at the same steps with and without the flag
    train_steps = lambda ls: [l["step"] for l in ls if "loss" in l]
    assert len(train_steps(lines)) >= 8 and train_steps(lines) == train_steps([json.loads(l) for l in off.stdout.splitlines() if l.startswith("{")])
