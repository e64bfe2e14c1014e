"""svla_action_metrics_f32 (csrc/metrics.hip; ops.action_metrics): the validation metrics of one batch in one launch, against the numpy / fp64 restatement of its
contract (tests/helpers/action_metrics_ref.py).

  * counts and sums[1] EXACTLY; sums[0] within 2e-6 * max(1, |want|) of the fp64 value (the gate tests/test_kernels_gpu.py::test_ce_loss_fwd_bwd_vs_torch uses for
    the same quantity); pred = torch.argmax over the valid columns; planted ties of two and three maxima, at indices 0 and A - 1 among them: the lowest index wins;
  * the accumulators accumulate: an all-ignored batch changes nothing, two launches on the halves of a batch leave the counts of one launch on the whole;
  * a target of A, a target of -7 and a row with a NaN among its A logits each add exactly 1 to sums[2] and touch nothing else (a sentinel behind counts stays);
  * pred = None; what ops.action_metrics refuses before any launch.
Shapes: rows in {1, 5, 1000} x A in {1, 20, 64}, ld = A + 3 with NaN in the three padding columns (they must not be read), about 30 % of the targets -1."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import action_metrics_ref as R      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(rows, A) for rows in (1, 5, 1000) for A in (1, 20, 64)]
SENTINEL = -0x0123456789ABCDEF


def _case(rows, A, seed, ignored=0.3):
    rs = np.random.RandomState(seed)
    x = (rs.standard_normal((rows, A)) * 1.5).astype(np.float32)
    t = rs.randint(0, A, rows).astype(np.int64)
    t[rs.uniform(size=rows) < ignored] = -1
    return x, t


def _state(A):
    """counts [A, A] with one sentinel word behind it, sums [3]"""
    buf = torch.zeros(A * A + 1, device=DEV, dtype=torch.int64)
    buf[A * A] = SENTINEL
    return buf, buf[:A * A].view(A, A), torch.zeros(3, device=DEV, dtype=torch.float64)


def _launch(x, t, counts, sums, with_pred=True, pad=3):
    """One launch on logits kept in a buffer whose rows are ld = A + pad apart, the padding NaN -> pred as numpy (or None)"""
    from safevla_amd import ops

    rows, A = x.shape
    buf = torch.full((rows, A + pad), float("nan"), device=DEV, dtype=torch.float32)
    buf[:, :A] = torch.from_numpy(x).to(DEV)
    pred = torch.full((rows,), -99, device=DEV, dtype=torch.int32) if with_pred else None
    ops.action_metrics(buf[:, :A], torch.from_numpy(t).to(DEV), counts, sums, ignore_index=-1, pred=pred, ld=A + pad)
    torch.cuda.synchronize()
    return None if pred is None else pred.cpu().numpy()


def _check(counts, sums, want_counts, want_sums, buf=None):
    got_s = sums.cpu().numpy()
    err, gate = abs(got_s[0] - want_sums[0]), 2e-6 * max(1.0, abs(want_sums[0]))
    print(f"sums[0] = {got_s[0]:.9f}, fp64 {want_sums[0]:.9f}: |diff| = {err:.3e}, gate {gate:.3e}; frames {got_s[1]:.0f}, refused {got_s[2]:.0f}")
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    assert got_s[1] == want_sums[1] and got_s[2] == want_sums[2]
    assert err <= gate
    if buf is not None:
        assert int(buf[-1]) == SENTINEL


@pytest.mark.parametrize("rows,A", SHAPES)
def test_counts_sums_and_pred_against_the_contract(rows, A):
    x, t = _case(rows, A, 100 * rows + A)
    if A > 3:                                                             # planted ties: two and three equal maxima, at indices 0 and A - 1 among them
        for r in range(rows):
            idx = {0: (0, A - 1), 1: (0, A // 2, A - 1), 2: (1, 2), 3: (A - 3, A - 2, A - 1)}.get(r % 5)
            if idx:
                x[r, list(idx)] = x[r].max() + 0.5
    buf, counts, sums = _state(A)
    pred = _launch(x, t, counts, sums)
    want_c, want_s, want_p = R.metrics(x, t)
    _check(counts, sums, want_c, want_s, buf)
    assert np.array_equal(pred, want_p)
    assert np.array_equal(pred, torch.argmax(torch.from_numpy(x), -1).numpy())
    if A > 3 and rows >= 5:
        assert pred[0] == 0 and pred[1] == 0 and pred[2] == 1 and pred[3] == A - 3
    assert int(want_s[1]) == int((t != -1).sum()) and counts.sum().item() == want_s[1]


def test_an_all_ignored_batch_changes_nothing():
    rows, A = 37, 20
    x, t = _case(rows, A, 1)
    buf, counts, sums = _state(A)
    _launch(x, t, counts, sums)
    before = (buf.clone(), sums.clone())
    pred = _launch(x, np.full(rows, -1, np.int64), counts, sums)
    assert torch.equal(buf, before[0]) and torch.equal(sums, before[1])
    assert np.array_equal(pred, np.argmax(x, 1))                          # pred is written for ignored rows too


def test_two_launches_on_halves_equal_one_on_the_whole():
    rows, A = 1000, 20
    x, t = _case(rows, A, 2)
    _, whole_c, whole_s = _state(A)
    _launch(x, t, whole_c, whole_s)
    buf, counts, sums = _state(A)
    _launch(x[:437], t[:437], counts, sums)
    _launch(x[437:], t[437:], counts, sums)
    assert torch.equal(counts, whole_c) and float(sums[1]) == float(whole_s[1])
    want_c, want_s, _ = R.metrics(x, t)
    _check(counts, sums, want_c, want_s, buf)


@pytest.mark.parametrize("what", ["target_A", "target_minus_7", "nan_logit"])
def test_refused_rows_add_one_to_sums2_and_nothing_else(what):
    rows, A = 9, 20
    x, t = _case(rows, A, 3, ignored=0.0)
    x[4, 7] = x[4].max() + 1.0                                            # the refused row's cell, were it counted: [t, 7]
    buf, counts, sums = _state(A)
    _launch(np.delete(x, 4, 0), np.delete(t, 4), counts, sums)            # the batch without the row: what must come out
    clean = (buf.clone(), sums.clone())
    if what == "target_A":
        t[4] = A
    elif what == "target_minus_7":
        t[4] = -7
    else:
        x[4, A - 1] = np.nan
    buf, counts, sums = _state(A)
    pred = _launch(x, t, counts, sums)
    assert torch.equal(buf, clean[0]) and int(buf[-1]) == SENTINEL
    assert sums[2].item() == 1.0 and sums[1].item() == rows - 1
    assert abs(sums[0].item() - clean[1][0].item()) <= 2e-6 * max(1.0, abs(clean[1][0].item()))
    want_c, want_s, want_p = R.metrics(x, t)
    _check(counts, sums, want_c, want_s, buf)
    assert np.array_equal(pred, want_p) and pred[4] == (-1 if what == "nan_logit" else 7)


def test_pred_none():
    rows, A = 5, 20
    x, t = _case(rows, A, 4)
    buf, counts, sums = _state(A)
    assert _launch(x, t, counts, sums, with_pred=False) is None
    want_c, want_s, _ = R.metrics(x, t)
    _check(counts, sums, want_c, want_s, buf)


def test_ops_action_metrics_refuses_before_any_launch():
    from safevla_amd import ops
    from safevla_amd._lib import lib

    rows, A = 6, 20
    logits = torch.zeros(rows, A, device=DEV)
    target = torch.zeros(rows, device=DEV, dtype=torch.int64)
    _, counts, sums = _state(A)
    bad = [
        (TypeError, dict(logits=logits.double())), (TypeError, dict(target=target.int())), (TypeError, dict(counts=counts.int())),
        (TypeError, dict(sums=sums.float())), (TypeError, dict(pred=torch.zeros(rows, device=DEV, dtype=torch.int64))),
        (ValueError, dict(logits=logits.cpu())), (ValueError, dict(target=target.cpu())), (ValueError, dict(counts=counts.cpu())), (ValueError, dict(sums=sums.cpu())),
        (ValueError, dict(counts=torch.zeros(A, A + 1, device=DEV, dtype=torch.int64))), (ValueError, dict(counts=torch.zeros(A * A, device=DEV, dtype=torch.int64))),
        (ValueError, dict(logits=torch.zeros(A, rows, device=DEV).t())),                                  # rows that are not dense
        (ValueError, dict(target=target[:5])), (ValueError, dict(sums=torch.zeros(2, device=DEV, dtype=torch.float64))),
    ]
    calls = lib().recorder = []
    try:
        for exc, over in bad:
            kw = dict(logits=logits, target=target, counts=counts, sums=sums)
            kw.update(over)
            with pytest.raises(exc):
                ops.action_metrics(**kw)
        assert calls == []                                                # no C-ABI call was made
        ops.action_metrics(logits, target, counts, sums)                  # the valid call
        assert [fn.__name__ for fn, _ in calls] == ["svla_action_metrics_f32"]
    finally:
        lib().recorder = None
    torch.cuda.synchronize()
    assert counts[0, 0].item() == rows and sums[1].item() == rows
