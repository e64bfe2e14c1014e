"""svla_policy_sample_rows_f32 (csrc/sample.hip; ops.policy_sample_rows): log-softmax, probabilities, greedy and sampled action of every row in one launch.

  * log_probs against an fp64 log_softmax: absolute error <= 1e-5 (an fp32 log-softmax of O(1) logits); measured on an MI355X: at most 7.8e-7 over the nine shapes;
  * greedy = argmax with the lowest index on ties;
  * sampled = EXACTLY the host replay of the contract (tests/helpers/policy_sample_ref.py: numpy mirror of the counter hash, sequential fp32 sums) on the probs the
    kernel wrote; an action of probability 0 is never returned; bitwise repeatable; the draw moves with the seed and with the age;
  * frequencies of one fixed 20-way distribution over 65 536 counters within 5 standard deviations (the seed is checked on the CPU by
    tests/test_policy_sample_cabi_cpu.py).
Shapes: n in {1, 5, 64} x A in {1, 20, 64}, ld > A."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import policy_sample_ref as R      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(n, A) for n in (1, 5, 64) for A in (1, 20, 64)]


def _run(logits_np, slot, age, seed, pad=3):
    """logits [n, A] -> the kernel's four outputs as numpy, read from a buffer whose rows are ld = A + pad apart (the padding holds NaN: it must not be read)"""
    from safevla_amd import ops

    n, A = logits_np.shape
    buf = torch.full((n, A + pad), float("nan"), device=DEV, dtype=torch.float32)
    buf[:, :A] = torch.from_numpy(logits_np).to(DEV)
    out = ops.policy_sample_rows(buf[:, :A], torch.as_tensor(slot, dtype=torch.int32).to(DEV), torch.as_tensor(age, dtype=torch.int32).to(DEV), seed, ld=A + pad)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def _logits(n, A, seed):
    rs = np.random.RandomState(seed)
    return (rs.standard_normal((n, A)) * 1.5).astype(np.float32), rs.randint(0, 1024, n).astype(np.int32), rs.randint(0, 1000, n).astype(np.int32)


@pytest.mark.parametrize("n,A", SHAPES)
def test_log_probs_probs_greedy_and_the_exact_replay(n, A):
    x, slot, age = _logits(n, A, 100 * n + A)
    if A > 2:                                                             # planted ties: the maximum twice, lowest index wins
        for r in range(0, n, 2):
            i, j = sorted(np.random.RandomState(r).choice(A, 2, replace=False))
            x[r, i] = x[r, j] = x[r].max() + 0.5
    lp, p, sampled, greedy = _run(x, slot, age, seed=11)
    ref = torch.log_softmax(torch.from_numpy(x).double(), -1).numpy()
    err = np.abs(lp - ref).max()
    print(f"n = {n}, A = {A}: max |log_probs - fp64 log_softmax| = {err:.3e}")
    assert err <= 1e-5
    assert np.abs(p - np.exp(ref)).max() <= 1e-6 and np.abs(p.sum(1) - 1.0).max() < 1e-5
    assert np.array_equal(greedy, np.argmax(x, 1))                        # numpy's argmax: the first of the maxima
    assert np.array_equal(sampled, R.sample(p, 11, slot, age))
    lp2, p2, s2, g2 = _run(x, slot, age, seed=11)
    for a, b in ((lp, lp2), (p, p2), (sampled, s2), (greedy, g2)):
        assert a.tobytes() == b.tobytes()                                 # bitwise repeatable


def test_zero_probability_actions_are_never_sampled():
    n, A = 64, 20
    x, _, _ = _logits(n, A, 5)
    x[:, [0, 7, A - 1]] = -999999.0                                       # first, interior, last: exp underflows to exactly 0
    x[n - 1, :] = -999999.0
    x[n - 1, 13] = 0.25                                                   # a row with a single non-zero action
    for rep in range(16):                                                 # 1024 draws
        slot, age = np.arange(n, dtype=np.int32), np.full(n, rep, np.int32)
        _, p, sampled, greedy = _run(x, slot, age, seed=3)
        assert (p[:, [0, 7, A - 1]] == 0).all() and p[n - 1, 13] == 1.0
        assert not np.isin(sampled, [0, 7, A - 1]).any() and sampled[n - 1] == 13 and greedy[n - 1] == 13
        assert np.array_equal(sampled, R.sample(p, 3, slot, age))
    # u close to 1 on a row whose last actions have probability 0: the draw falls on an action that has probability
    big = np.where(R.bits24(3, np.zeros(1 << 16, np.int64), np.arange(1 << 16)) >= (1 << 24) - (1 << 14))[0][:8]      # 64 of them expected
    assert big.size == 8
    _, p, sampled, _ = _run(np.repeat(x[:1], big.size, 0), np.zeros(big.size, np.int32), big.astype(np.int32), seed=3)
    assert (p[np.arange(big.size), sampled] > 0).all() and np.array_equal(sampled, R.sample(p, 3, np.zeros(big.size), big))


def test_the_draw_moves_with_seed_and_age_only():
    n, A = 64, 64
    x = np.zeros((n, A), np.float32)                                      # uniform over 64 actions: the draw shows the counter
    slot, age = np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32) * 3
    base = _run(x, slot, age, seed=1)[2]
    assert not np.array_equal(base, _run(x, slot, age, seed=2)[2])
    assert not np.array_equal(base, _run(x, slot, age + 1, seed=1)[2])
    assert not np.array_equal(base, _run(x, slot + 1, age, seed=1)[2])
    perm = np.random.RandomState(0).permutation(n)                        # a row's draw does not depend on where it sits or on who else is in the launch
    assert np.array_equal(base[perm], _run(x[perm], slot[perm], age[perm], seed=1)[2])
    assert np.array_equal(base[:5], _run(x[:5], slot[:5], age[:5], seed=1)[2])


def test_frequencies_of_a_fixed_distribution():
    slot, age = R.freq_counters()
    x = np.tile(np.log(R.FREQ_PROBS).astype(np.float32), (slot.shape[0], 1))
    _, p, sampled, _ = _run(x, slot, age, seed=R.FREQ_SEED)
    assert np.abs(p[0].astype(np.float64) - R.FREQ_PROBS).max() < 1e-6 and p.min() >= 0.0099
    z, counts = R.freq_check(sampled, p[0])
    print(f"worst deviation {z:.2f} standard deviations; counts {counts.tolist()}")
    assert z < 5.0, (z, counts)
    assert np.array_equal(sampled, R.sample(p, R.FREQ_SEED, slot, age))
