"""What svla_policy_sample_rows_f32 (include/svla.h, csrc/sample.hip) refuses: host checks that return SVLA_EINVAL (-1) before any launch, so they hold on a machine
without a GPU (the mechanism of tests/test_attn_cabi_cpu.py; the GPU side is in tests/test_policy_sample_gpu.py).  Plus, with the numpy mirror of the counter hash
alone (tests/helpers/policy_sample_ref.py), that the seed and the distribution of the GPU frequency test satisfy that test's condition."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import policy_sample_ref as R      # noqa: E402

NAME = "svla_policy_sample_rows_f32"


@pytest.fixture(scope="module")
def lib():
    from safevla_amd import build
    from safevla_amd._lib import parse_header

    cdll = ctypes.CDLL(build.build())
    decls = parse_header()
    fn = getattr(cdll, NAME)
    fn.restype, fn.argtypes = ctypes.c_int, [ct for _, ct in decls[NAME]]
    return cdll, decls


def _call(lib, **over):
    cdll, decls = lib
    base = dict(logits=64, ld=24, slot=64, age=64, seed=7, n=5, A=20, log_probs=64, probs=64, sampled=64, greedy=64, stream=None)
    assert [n for n, _ in decls[NAME]] == list(base), decls[NAME]          # the argument order of the header
    base.update(over)
    return getattr(cdll, NAME)(*base.values())


@pytest.mark.parametrize("over", [dict(n=0), dict(n=-3), dict(A=0), dict(A=65), dict(ld=19), dict(slot=None), dict(age=None), dict(logits=None), dict(log_probs=None),
                                  dict(probs=None), dict(sampled=None), dict(greedy=None)])
def test_policy_sample_rows_refusals(lib, over):
    assert _call(lib, **over) == -1


def test_mix24_mirror_matches_the_header_by_hand():
    """mix24(1), one line at a time as include/svla.h writes it, in Python integers"""
    x = 1
    x ^= x >> 16; x = ((x & 0xFFFFFF) * 0xEB352D) & 0xFFFFFFFF; x ^= x >> 13; x = ((x & 0xFFFFFF) * 0x6CA68B) & 0xFFFFFFFF; x ^= x >> 16      # noqa: E702
    assert int(R.mix24(np.array([1]))[0]) == x
    big = 0xFEDCBA98
    y = big ^ (big >> 16); y = ((y & 0xFFFFFF) * 0xEB352D) & 0xFFFFFFFF; y ^= y >> 13; y = ((y & 0xFFFFFF) * 0x6CA68B) & 0xFFFFFFFF; y ^= y >> 16      # noqa: E702
    assert int(R.mix24(np.array([big]))[0]) == y
    u = R.uniform(5, np.arange(4), np.arange(4))
    assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()
    assert R.bits24(-1, [-1], [-2]) == R.bits24(0xFFFFFFFF, [0xFFFFFFFF], [0xFFFFFFFE])      # taken as their 32 bits


def test_frequency_condition_holds_for_the_committed_seed_on_the_cpu():
    assert abs(R.FREQ_PROBS.sum() - 1.0) < 1e-12 and R.FREQ_PROBS.min() >= 0.01 and R.FREQ_PROBS.shape == (20,)
    slot, age = R.freq_counters()
    probs = np.tile(R.FREQ_PROBS.astype(np.float32), (slot.shape[0], 1))
    sampled = R.sample(probs, R.FREQ_SEED, slot, age)
    z, counts = R.freq_check(sampled, probs[0])
    print(f"seed {R.FREQ_SEED}: worst deviation {z:.2f} sigma; counts {counts.tolist()}")
    assert counts.sum() == 65536 and z < 5.0, (z, counts)
