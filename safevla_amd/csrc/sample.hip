// Policy read-out of an acting step in one launch: log-softmax, probabilities, the greedy action and one sampled action per row (svla_policy_sample_rows_f32; the
// contract is in include/svla.h).  Replaces log_softmax + exp + multinomial + argmax of CategoricalDistr (utils/nn_utils.py sample_action_index_from_logits;
// AllenAct CategoricalDistr [3P]) for the vector agent: the draw of a row is a pure function of (seed, slot, age), so it does not depend on who shares the batch.
// One wave per row, lane k = action k (A <= 64); four rows per workgroup; no LDS, no atomics: every output is a plain store, bitwise repeatable.
#include "common.h"

#define SAMPLE_WAVES 4

// 24 uniform bits of the counter (seed, slot, age): two rounds of the dropout mixer (drop_mix = mix24 of include/svla.h), top 24 bits of the second
__device__ __forceinline__ unsigned sample_bits24(unsigned seed, unsigned slot, unsigned age) {
    const unsigned h = drop_mix(seed ^ slot * 0x9E3779B1u);
    return drop_mix(h ^ age * 0x85EBCA77u ^ 0xC2B2AE3Du) >> 8;
}

__global__ void __launch_bounds__(64 * SAMPLE_WAVES) policy_sample_rows_kernel(const float* __restrict__ logits, long ld, const int* __restrict__ slot,
                                                                                const int* __restrict__ age, unsigned seed, int n, int A,
                                                                                float* __restrict__ log_probs, float* __restrict__ probs,
                                                                                int* __restrict__ sampled, int* __restrict__ greedy) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * SAMPLE_WAVES + (threadIdx.x >> 6);
    if (row >= n) return;                                                  // wave-uniform
    const bool on = lane < A;
    const float x = on ? logits[(size_t)row * ld + lane] : -INFINITY;
    const float mx = wave_max(x);
    const float se = wave_sum(on ? expf(x - mx) : 0.f);                    // the xor butterfly leaves the same bits in every lane
    const float lp = x - (mx + logf(se));
    const float p = on ? expf(lp) : 0.f;
    if (on) {
        log_probs[(size_t)row * A + lane] = lp;
        probs[(size_t)row * A + lane] = p;
    }
    const unsigned long long is_max = __ballot(on && x == mx);
    const int g = is_max ? __ffsll((long long)is_max) - 1 : 0;            // lowest index of the maximum (no lane equals a NaN maximum: action 0)
    // c_k = probs[0] + ... + probs[k], added in action order: lane k takes the first k + 1 terms, and adding 0.f leaves a sum as it is
    float c = 0.f;
    for (int j = 0; j < A; ++j) {
        const float pj = __shfl(p, j, 64);
        c += j <= lane ? pj : 0.f;
    }
    const float total = __shfl(c, A - 1, 64);
    const float u = (float)sample_bits24(seed, (unsigned)slot[row], (unsigned)age[row]) * 0x1p-24f;     // exact: 24 bits
    const float thr = u * total;
    const unsigned long long pos = __ballot(on && p > 0.f);
    const unsigned long long hit = __ballot(on && p > 0.f && c > thr);
    int s = g;                                                             // no action with probs > 0 (NaN logits): the greedy index
    if (hit) s = __ffsll((long long)hit) - 1;
    else if (pos) s = 63 - __clzll((long long)pos);
    if (lane == 0) {
        sampled[row] = s;
        greedy[row] = g;
    }
}

extern "C" int svla_policy_sample_rows_f32(const float* logits, long ld, const int* slot, const int* age, int seed, int n, int A, float* log_probs,
                                           float* probs, int* sampled, int* greedy, void* stream) {
    if (n <= 0 || A < 1 || A > 64 || ld < A || !logits || !slot || !age || !log_probs || !probs || !sampled || !greedy) return SVLA_EINVAL;
    return svla_launch<policy_sample_rows_kernel>(dim3((n + SAMPLE_WAVES - 1) / SAMPLE_WAVES), dim3(64 * SAMPLE_WAVES), 0, (hipStream_t)stream, logits, ld, slot, age,
                                                  (unsigned)seed, n, A, log_probs, probs, sampled, greedy);
}
