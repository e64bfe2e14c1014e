"""Host restatement of the contract of svla_action_metrics_f32 (include/svla.h) in numpy / fp64, and of the F1 arithmetic behind il.f1_from_counts.  Imports nothing
of safevla_amd: what the tests compare against is written here once, from the contract's text."""
import numpy as np


def metrics(logits, target, A=None, ignore_index=-1, counts=None, sums=None):
    """logits [rows, >= A] (the first A columns are read), target [rows] -> (counts [A, A] int64, sums [3] fp64, pred [rows] int32).  ``counts`` / ``sums`` given:
    the accumulators to add to (copies are returned).  Row by row, as the contract states it."""
    logits = np.asarray(logits, dtype=np.float64)
    target = np.asarray(target, dtype=np.int64)
    A = logits.shape[1] if A is None else A
    counts = np.zeros((A, A), np.int64) if counts is None else np.array(counts, dtype=np.int64)
    sums = np.zeros(3, np.float64) if sums is None else np.array(sums, dtype=np.float64)
    pred = np.empty(logits.shape[0], np.int32)
    for r in range(logits.shape[0]):
        x, t = logits[r, :A], int(target[r])
        nan = bool(np.isnan(x).any())
        p = -1 if nan else int(np.flatnonzero(x == x.max())[0])         # the lowest index of the maximum
        pred[r] = p
        if t == ignore_index:
            continue
        if nan or not 0 <= t < A:
            sums[2] += 1
            continue
        m = x.max()
        counts[t, p] += 1
        sums[0] += (m + np.log(np.exp(x - m).sum())) - x[t]
        sums[1] += 1
    return counts, sums, pred


def f1(C):
    """Confusion matrix C[target, pred] -> (per-class F1 [A], macro, weighted), class by class in Python floats:
    f1_k = 2 tp / (2 tp + fp + fn), 0 where the denominator is 0; macro over the classes with tp + fp + fn > 0; weighted by the support tp + fn; 0.0 when no class
    qualifies."""
    C = np.asarray(C)
    A = C.shape[0]
    per, seen, support = [], [], []
    for k in range(A):
        tp = int(C[k, k])
        fp = int(C[:, k].sum()) - tp
        fn = int(C[k, :].sum()) - tp
        den = 2 * tp + fp + fn
        per.append(2.0 * tp / den if den else 0.0)
        seen.append(den > 0)
        support.append(tp + fn)
    n_seen, n_sup = sum(seen), sum(support)
    macro = sum(v for v, s in zip(per, seen) if s) / n_seen if n_seen else 0.0
    weighted = sum(w * v for w, v in zip(support, per)) / n_sup if n_sup else 0.0
    return np.array(per), macro, weighted
