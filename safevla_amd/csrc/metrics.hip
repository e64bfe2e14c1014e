// Validation metrics of the imitation-learning trainer in one launch per batch (svla_action_metrics_f32; the contract is in include/svla.h): the greedy action of
// every row, the confusion matrix counts[target, pred] behind the three F1Score objects of LitModel.validation_step (training/offline/train_pl.py:187-207,252-259)
// and the summed cross-entropy of nn.CrossEntropyLoss(ignore_index=-1) (early_fusion_tsfm_models.py:88,117-119).  Replaces argmax + F.cross_entropy + bincount and
// the host read per batch: counts and sums are accumulators that stay in device memory until the epoch ends.
// One wave per row, lane k = action k (A <= 64), as in sample.hip; four waves per workgroup, each striding over the rows.  A workgroup keeps an A x A int histogram
// in LDS and one fp64 partial per wave and sum, and ends with one global add per non-zero cell and per non-zero sum.
#include "common.h"

#define METRICS_WAVES 4
#define METRICS_MAX_A 64
#define METRICS_MAX_BLOCKS 256      // one workgroup per compute unit of an MI355X is plenty: a validation batch has 800 ... 16 000 rows

__global__ void __launch_bounds__(64 * METRICS_WAVES) action_metrics_kernel(const float* __restrict__ logits, long ld, const long* __restrict__ target, int rows, int A,
                                                                             long ignore_index, long long* __restrict__ counts, double* __restrict__ sums,
                                                                             int* __restrict__ pred) {
    __shared__ int hist[METRICS_MAX_A * METRICS_MAX_A];                    // 16 KiB; the first A * A cells are used
    __shared__ double part[METRICS_WAVES][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cells = A * A;
    for (int i = threadIdx.x; i < cells; i += 64 * METRICS_WAVES) hist[i] = 0;
    __syncthreads();
    const bool on = lane < A;
    const int stride = gridDim.x * METRICS_WAVES;
    double loss = 0.0, valid = 0.0, refused = 0.0;                         // wave-uniform
    long row = blockIdx.x * METRICS_WAVES + wave;                          // row, and with it every branch below, is wave-uniform (long: row + stride may pass 2^31)
    float x = 0.f;
    long t = 0;
    if (row < rows) {
        x = on ? logits[(size_t)row * ld + lane] : -INFINITY;
        t = target[row];
    }
    while (row < rows) {
        const long next = row + stride;                                    // the next row's loads are in flight while this one is reduced
        float xn = 0.f;
        long tn = 0;
        if (next < rows) {
            xn = on ? logits[(size_t)next * ld + lane] : -INFINITY;
            tn = target[next];
        }
        const bool has_nan = __ballot(on && x != x) != 0ull;
        const float mx = wave_max(x);
        const unsigned long long is_max = __ballot(on && x == mx);
        const int p = has_nan || !is_max ? -1 : __ffsll((long long)is_max) - 1;      // lowest index of the maximum: 0 <= p < A
        if (pred && lane == 0) pred[row] = p;
        if (t != ignore_index) {
            if (p < 0 || t < 0 || t >= (long)A) {
                refused += 1.0;
            } else {
                const float se = wave_sum(on ? expf(x - mx) : 0.f);        // the xor butterfly leaves the same bits in every lane
                const float xt = __shfl(x, (int)t, 64);
                loss += (double)(mx + logf(se)) - (double)xt;
                valid += 1.0;
                if (lane == 0) atomicAdd(&hist[(int)t * A + p], 1);
            }
        }
        row = next; x = xn; t = tn;
    }
    if (lane == 0) { part[wave][0] = loss; part[wave][1] = valid; part[wave][2] = refused; }
    __syncthreads();
    for (int i = threadIdx.x; i < cells; i += 64 * METRICS_WAVES) {
        const int c = hist[i];
        if (c) atomicAdd((unsigned long long*)(counts + i), (unsigned long long)c);
    }
    if (threadIdx.x < 3) {
        double s = 0.0;
        for (int w = 0; w < METRICS_WAVES; ++w) s += part[w][threadIdx.x];
        if (s != 0.0) atomicAdd(sums + threadIdx.x, s);                    // (a NaN sum compares unequal to 0 and is added: a diverged loss stays visible)
    }
}

extern "C" int svla_action_metrics_f32(const float* logits, long ld, const long* target, int rows, int A, long ignore_index, long long* counts, double* sums,
                                       int* pred, void* stream) {
    if (rows <= 0 || A < 1 || A > METRICS_MAX_A || ld < A || !logits || !target || !counts || !sums) return SVLA_EINVAL;
    const int need = (rows - 1) / METRICS_WAVES + 1;
    return svla_launch<action_metrics_kernel>(dim3(need < METRICS_MAX_BLOCKS ? need : METRICS_MAX_BLOCKS), dim3(64 * METRICS_WAVES), 0, (hipStream_t)stream, logits, ld,
                                              target, rows, A, ignore_index, counts, sums, pred);
}
