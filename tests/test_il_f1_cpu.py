"""il.f1_from_counts and the host side of il.ActionF1, without a GPU.

The F1 arithmetic (torchmetrics' multiclass F1Score restated, unpinned: see il.f1_from_counts) against the class-by-class restatement of
tests/helpers/action_metrics_ref.py and, where sklearn is installed, against sklearn.metrics.f1_score(labels=None) for average = None / "macro" / "weighted".
ActionF1 on CPU tensors: compute() refuses a state with refused rows, reset(), and reduce_() under a 2-rank gloo group (started as tests/test_parallel_cpu.py starts
its ranks) leaves the sum of the two states on both ranks."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import action_metrics_ref as R      # noqa: E402


def _check(C):
    from safevla_amd import il

    got = il.f1_from_counts(C)
    per, macro, weighted = R.f1(C)
    assert len(got["f1"]) == len(per) and not np.isnan(got["f1"]).any()
    assert np.abs(np.array(got["f1"]) - per).max() <= 1e-12 and abs(got["f1_macro"] - macro) <= 1e-12 and abs(got["f1_weighted"] - weighted) <= 1e-12, (got, per)
    return got


def _random_confusion(rs, A, n, drop_target=(), drop_pred=()):
    t, p = rs.randint(0, A, n), rs.randint(0, A, n)
    keep = ~np.isin(t, drop_target) & ~np.isin(p, drop_pred)
    C = np.zeros((A, A), np.int64)
    np.add.at(C, (t[keep], p[keep]), 1)
    return C, t[keep], p[keep]


def test_random_matrices_numpy_and_torch_input():
    from safevla_amd import il

    rs = np.random.RandomState(0)
    for A in (2, 5, 20):
        C, _, _ = _random_confusion(rs, A, 400)
        got = _check(C)
        assert il.f1_from_counts(torch.from_numpy(C)) == got


def test_absent_class_leaves_the_macro_mean_unchanged():
    rs = np.random.RandomState(1)
    C, _, _ = _random_confusion(rs, 6, 300)
    wide = np.zeros((7, 7), np.int64)                 # class 6: in neither targets nor predictions
    wide[:6, :6] = C
    a, b = _check(C), _check(wide)
    assert b["f1"][6] == 0.0 and abs(a["f1_macro"] - b["f1_macro"]) <= 1e-15 and abs(a["f1_weighted"] - b["f1_weighted"]) <= 1e-15


def test_class_that_is_only_predicted_enters_the_macro_mean_with_zero():
    C = np.array([[5, 0, 2], [0, 4, 1], [0, 0, 0]], np.int64)      # class 2: predicted three times, never a target
    got = _check(C)
    assert got["f1"][2] == 0.0
    assert abs(got["f1_macro"] - (got["f1"][0] + got["f1"][1] + 0.0) / 3) <= 1e-15
    assert abs(got["f1_weighted"] - (7 * got["f1"][0] + 5 * got["f1"][1]) / 12) <= 1e-15      # no support: no weight


def test_class_with_support_that_is_never_predicted():
    C = np.array([[6, 1, 0], [2, 3, 0], [1, 3, 0]], np.int64)      # class 2: four targets, no prediction
    got = _check(C)
    assert got["f1"][2] == 0.0
    assert abs(got["f1_macro"] - (got["f1"][0] + got["f1"][1]) / 3) <= 1e-15
    assert abs(got["f1_weighted"] - (7 * got["f1"][0] + 5 * got["f1"][1] + 4 * 0.0) / 16) <= 1e-15


def test_all_zero_matrix_gives_zero_and_no_nan():
    got = _check(np.zeros((20, 20), np.int64))
    assert got["f1"] == [0.0] * 20 and got["f1_macro"] == 0.0 and got["f1_weighted"] == 0.0


def test_a_single_class():
    assert _check(np.array([[7]], np.int64)) == dict(f1=[1.0], f1_macro=1.0, f1_weighted=1.0)
    assert _check(np.array([[0]], np.int64)) == dict(f1=[0.0], f1_macro=0.0, f1_weighted=0.0)


def test_against_sklearn():
    sk = pytest.importorskip("sklearn.metrics")
    from safevla_amd import il

    rs = np.random.RandomState(2)
    for i in range(40):
        A = int(rs.randint(2, 21))
        drop_t = rs.choice(A, rs.randint(0, max(1, A // 3)), replace=False)      # classes that occur only in the predictions ...
        drop_p = rs.choice(A, rs.randint(0, max(1, A // 3)), replace=False)      # ... and only in the targets
        C, t, p = _random_confusion(rs, A, 200, drop_t, drop_p)
        got = il.f1_from_counts(C)
        labels = np.union1d(t, p)                                                # labels=None: the classes that occur, sorted
        assert np.abs(np.array(got["f1"])[labels] - sk.f1_score(t, p, average=None, zero_division=0)).max() <= 1e-12
        assert abs(got["f1_macro"] - sk.f1_score(t, p, average="macro", zero_division=0)) <= 1e-12
        assert abs(got["f1_weighted"] - sk.f1_score(t, p, average="weighted", zero_division=0)) <= 1e-12


def _filled(A, seed):
    """An ActionF1 on CPU tensors with a planted state"""
    from safevla_amd import il

    rs = np.random.RandomState(seed)
    m = il.ActionF1(A, -1, device="cpu")
    m.counts.copy_(torch.from_numpy(rs.randint(0, 50, (A, A))))
    m.sums.copy_(torch.tensor([rs.uniform(10, 20), float(m.counts.sum()), 0.0], dtype=torch.float64))
    return m


def test_action_f1_compute_raises_on_refused_rows_and_reset():
    m = _filled(20, 3)
    assert m.counts.dtype == torch.int64 and m.sums.dtype == torch.float64 and m.counts.shape == (20, 20) and m.sums.shape == (3,)
    out = m.compute()
    per, macro, weighted = R.f1(m.counts.numpy())
    assert np.abs(np.array(out["f1"]) - per).max() <= 1e-12 and abs(out["f1_macro"] - macro) <= 1e-12 and abs(out["f1_weighted"] - weighted) <= 1e-12
    assert out["frames"] == int(m.counts.sum()) and abs(out["loss"] - float(m.sums[0]) / out["frames"]) <= 1e-15
    assert out["confusion"].dtype == np.int64 and np.array_equal(out["confusion"], m.counts.numpy())
    m.sums[2] = 3.0
    with pytest.raises(ValueError, match="3 rows"):
        m.compute()
    m.reset()
    assert int(m.counts.abs().sum()) == 0 and m.sums.tolist() == [0.0, 0.0, 0.0]
    out = m.compute()                                 # an empty epoch: zeros, no NaN
    assert out["loss"] == 0.0 and out["frames"] == 0 and out["f1_macro"] == 0.0 and out["f1_weighted"] == 0.0
    from safevla_amd import il
    with pytest.raises(ValueError):
        il.ActionF1(65, device="cpu")


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist

    from safevla_amd import parallel

    parallel.init_from_env(backend="gloo")
    m = _filled(5, 10 + rank)
    m.reduce_()
    q.put((rank, m.counts.numpy().copy(), m.sums.numpy().copy()))
    parallel.barrier()
    dist.destroy_process_group()


def test_reduce_sums_the_states_of_two_gloo_ranks():
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict((r, (c, s)) for r, c, s in (q.get(timeout=180) for _ in range(2)))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    a, b = _filled(5, 10), _filled(5, 11)
    for r in range(2):
        assert np.array_equal(got[r][0], (a.counts + b.counts).numpy())
        assert np.array_equal(got[r][1], (a.sums + b.sums).numpy())      # (two terms: one rounding, the same on both ranks)
    single = _filled(5, 10)
    single.reduce_()                                  # a single process: a no-op
    assert torch.equal(single.counts, a.counts) and torch.equal(single.sums, a.sums)
