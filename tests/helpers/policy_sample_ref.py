"""Host replay of the sampling contract of svla_policy_sample_rows_f32 (include/svla.h): a numpy mirror of the mix24 counter hash and of the inverse-CDF draw
over the probabilities the kernel wrote.  Integer arithmetic is mod 2^32, float arithmetic is fp32, in the kernel's order: the replay is exact."""
import numpy as np

_M32 = np.uint64(0xFFFFFFFF)


def mix24(x):
    """mix24 of include/svla.h on uint32 arrays (kept in uint64, reduced mod 2^32 after every multiply)"""
    x = np.asarray(x, dtype=np.uint64) & _M32
    x = x ^ (x >> np.uint64(16))
    x = ((x & np.uint64(0xFFFFFF)) * np.uint64(0xEB352D)) & _M32
    x = x ^ (x >> np.uint64(13))
    x = ((x & np.uint64(0xFFFFFF)) * np.uint64(0x6CA68B)) & _M32
    return x ^ (x >> np.uint64(16))


def bits24(seed, slot, age):
    """r of the contract: 24 uniform bits of the counter (seed, slot, age); slot, age: integer arrays (taken as their 32 bits)"""
    slot = np.asarray(slot, dtype=np.int64).astype(np.uint64) & _M32
    age = np.asarray(age, dtype=np.int64).astype(np.uint64) & _M32
    h = mix24(np.uint64(int(seed) & 0xFFFFFFFF) ^ ((slot * np.uint64(0x9E3779B1)) & _M32))
    return (mix24(h ^ ((age * np.uint64(0x85EBCA77)) & _M32) ^ np.uint64(0xC2B2AE3D)) >> np.uint64(8)).astype(np.uint32)


def uniform(seed, slot, age):
    return bits24(seed, slot, age).astype(np.float32) * np.float32(2.0 ** -24)


def sample(probs, seed, slot, age):
    """probs [n, A] fp32 as written by the kernel -> sampled [n]: the smallest k with c_k > u * c_{A-1} and probs[k] > 0, else the last k with probs[k] > 0
    (a row without one: -1; the kernel returns its greedy index there)"""
    probs = np.asarray(probs, dtype=np.float32)
    n, A = probs.shape
    c = np.zeros(n, np.float32)
    cum = np.empty((n, A), np.float32)
    for k in range(A):                                                   # sequential fp32 sum in action order
        c = (c + probs[:, k]).astype(np.float32)
        cum[:, k] = c
    thr = (uniform(seed, slot, age) * cum[:, A - 1]).astype(np.float32)
    pos = probs > 0
    hit = pos & (cum > thr[:, None])
    last = np.where(pos.any(1), A - 1 - np.argmax(pos[:, ::-1], 1), -1)
    return np.where(hit.any(1), np.argmax(hit, 1), last).astype(np.int64)


# the one fixed 20-way distribution, seed and counter grid of the frequency test (checked on the CPU by tests/test_policy_sample_cabi_cpu.py, on the GPU by tests/test_policy_sample_gpu.py)
FREQ_SEED = 2024
FREQ_PROBS = np.array([0.01, 0.02, 0.03, 0.04, 0.05, 0.06, 0.07, 0.08, 0.09, 0.10, 0.10, 0.09, 0.08, 0.06, 0.04, 0.03, 0.02, 0.01, 0.01, 0.01], np.float64)


def freq_counters():
    """65 536 (slot, age) counters: 64 slots x 1024 ages"""
    slot, age = np.meshgrid(np.arange(64), np.arange(1024), indexing="ij")
    return slot.reshape(-1).astype(np.int32), age.reshape(-1).astype(np.int32)


def freq_check(sampled, probs_row):
    """every action's count within 5 standard deviations of its binomial expectation -> (worst deviation in standard deviations, counts)"""
    n = sampled.shape[0]
    p = probs_row.astype(np.float64) / probs_row.astype(np.float64).sum()
    counts = np.bincount(sampled, minlength=p.shape[0])
    z = np.abs(counts - n * p) / np.sqrt(n * p * (1 - p))
    return float(z.max()), counts
