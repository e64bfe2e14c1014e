// Per-row KV rings of the llama decoder's acting step (include/svla.h: svla_kv_append_rows_bf16, svla_attn_decode_rows_bf16), bf16, head_dim 64: every row of a
// call is an episode of its own, with its own cache row, its own slot to write and its own number of keys to read.  A vector of evaluation episodes that start,
// end and stall independently is served by one set of weights and one call per layer; the slot and the length come from device memory, so the arguments of a call
// do not depend on the step.
//
// The attention kernel has the contract and the arithmetic of attn_decode_kernel (csrc/attn.hip) and attn_decode_long_kernel (csrc/attn_decode_long.hip): one
// query per row, bf16 products, fp32 accumulation, probabilities rounded to bf16 before the product with V, optional LSE (natural log), zeros for a row without a
// key.  Layout of attn_decode_long_kernel: one workgroup of 256 threads per (row, head), thread (g = tid / 8, c = tid % 8) owns the 16-byte chunk c of key 32 b + g of
// block b, DECL_U blocks of loads in flight per trip, scores in LDS between the two passes.  What differs: the valid keys are the prefix [0, min(klen[r], kv_rows))
// of cache row cache_row[r], so there are no validity bytes and no ballot -- the block count comes from klen and only the last block is partial.  The cost follows
// klen[r], not kv_rows.
#include "attn_common.h"      // LOG2E / LN2; common.h: bf16 helpers, SVLA_LAUNCH

#define HD 64
#define DECR_THREADS 256
#define DECR_U 8              // blocks per trip: 8 x 16 bytes per thread in flight
#define DECR_MAXS 1024        // keys of the longest ring (the LDS score array)

struct DecRowsArgs {
    const bf16_t *Q, *K, *V; long ld;
    bf16_t* O; long ldo;
    float* LSE;                           // [rows, H] or null
    const int* klen;                      // [rows]
    const int* cache_row;                 // [rows] or null (identity)
    int H;
    float scale;
    int kv_rows;
    long ldq;
};

__device__ __forceinline__ void attn_decode_rows_kernel_body(DecRowsArgs p) {
    __shared__ float ps[DECR_MAXS];              // scaled scores (log2 domain) of the keys of the blocks in use; -inf: beyond the row's length
    __shared__ float red[4][2];
    __shared__ float accs[4][64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int g = tid >> 3, c = tid & 7;
    const int r = blockIdx.x / p.H, h = blockIdx.x % p.H;
    // the row's length and cache row: the same for the whole workgroup
    const int n = __builtin_amdgcn_readfirstlane(min(p.klen[r], p.kv_rows));
    const int cr = __builtin_amdgcn_readfirstlane(p.cache_row ? p.cache_row[r] : r);
    const int nb = n > 0 ? (n + 31) >> 5 : 0;      // 32-key blocks; only the last one is partial
    const size_t tok0 = (size_t)cr * p.kv_rows;
    const float sl2 = p.scale * LOG2E;
    float qv[8];
    {
        const bf16x8 q8 = *(const bf16x8*)(p.Q + (size_t)r * p.ldq + h * HD + c * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) qv[e] = bf2f((bf16_t)q8[e]);
    }
    // ---- pass 1: scores of blocks [0, nb) -> LDS, running maximum
    float mx = -INFINITY;
    for (int b0 = 0; b0 < nb; b0 += DECR_U) {
        bool ok[DECR_U];
        bf16x8 k8[DECR_U];
#pragma unroll
        for (int u = 0; u < DECR_U; ++u) {
            const int key = (b0 + u) * 32 + g;
            ok[u] = key < n;                                  // (false for every block at or beyond nb)
            k8[u] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
            if (ok[u]) k8[u] = *(const bf16x8*)(p.K + (tok0 + key) * p.ld + h * HD + c * 8);
        }
#pragma unroll
        for (int u = 0; u < DECR_U; ++u) {
            if (b0 + u < nb) {                                // wave-uniform
                float d = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) d = fmaf(qv[e], bf2f((bf16_t)k8[u][e]), d);
                // the eight lanes of a key hold its eight partial dot products (ok is uniform over them)
                d += __shfl_xor(d, 1, 64); d += __shfl_xor(d, 2, 64); d += __shfl_xor(d, 4, 64);
                const float s = ok[u] ? d * sl2 : -INFINITY;
                if (c == 0) ps[(b0 + u) * 32 + g] = s;
                mx = fmaxf(mx, s);
            }
        }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 8, 64)); mx = fmaxf(mx, __shfl_xor(mx, 16, 64)); mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    if (lane == 0) red[wid][0] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0][0], red[1][0]), fmaxf(red[2][0], red[3][0]));
    if (mx == -INFINITY) mx = 0.f;
    // ---- pass 2: probabilities and P.V over the same blocks
    float acc[8], lsum = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    for (int b0 = 0; b0 < nb; b0 += DECR_U) {
        float s[DECR_U];
        bf16x8 v8[DECR_U];
#pragma unroll
        for (int u = 0; u < DECR_U; ++u) {
            const int key = (b0 + u) * 32 + g;
            s[u] = b0 + u < nb ? ps[key] : -INFINITY;
            // every lane loads, a key beyond n from key 0 of the row (n >= 1 inside this loop; the line is in cache), and the value is dropped by a select: with a
            // load under the lanes' own condition the compiler moves the bf16 unpacking up into each load's branch and waits for every load by itself
            const bf16x8 ld8 = *(const bf16x8*)(p.V + (tok0 + (key < n ? key : 0)) * p.ld + h * HD + c * 8);
            v8[u] = key < n ? ld8 : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        }
#pragma unroll
        for (int u = 0; u < DECR_U; ++u) {
            if (b0 + u < nb) {                                // wave-uniform; a key beyond n has s = -inf and v = 0 and adds exactly nothing
                const float pr = __builtin_amdgcn_exp2f(s[u] - mx);
                lsum += pr;
                const float pb = bf2f(f2bf(pr));                         // the MFMA path's operand rounding
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] = fmaf(pb, bf2f((bf16_t)v8[u][e]), acc[e]);
            }
        }
    }
    // every key was counted by its eight lanes: sum over lanes / 8; the accumulators: over the lanes that share chunk c
    lsum += __shfl_xor(lsum, 1, 64); lsum += __shfl_xor(lsum, 2, 64); lsum += __shfl_xor(lsum, 4, 64);
    lsum += __shfl_xor(lsum, 8, 64); lsum += __shfl_xor(lsum, 16, 64); lsum += __shfl_xor(lsum, 32, 64);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float a = acc[e];
        a += __shfl_xor(a, 8, 64); a += __shfl_xor(a, 16, 64); a += __shfl_xor(a, 32, 64);
        acc[e] = a;
    }
    if (lane == 0) red[wid][1] = lsum * 0.125f;
    if (lane < 8) {
#pragma unroll
        for (int e = 0; e < 8; ++e) accs[wid][lane * 8 + e] = acc[e];
    }
    __syncthreads();
    if (tid < 64) {
        const float ls = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
        const float o = (accs[0][tid] + accs[1][tid]) + (accs[2][tid] + accs[3][tid]);
        const float inv = ls > 0.f ? 1.f / ls : 0.f;
        p.O[(size_t)r * p.ldo + h * HD + tid] = f2bf(o * inv);
        if (p.LSE && tid == 0) p.LSE[(size_t)r * p.H + h] = (mx + __log2f(ls)) * LN2;
    }
}
__global__ void __launch_bounds__(DECR_THREADS) attn_decode_rows_kernel(DecRowsArgs p) { attn_decode_rows_kernel_body(p); }

extern "C" int svla_attn_decode_rows_bf16(const bf16_t* Q, long ldq, const bf16_t* K, const bf16_t* V, long ld, bf16_t* O, long ldo, float* LSE, const int* klen,
                                          const int* cache_row, int rows, int H, int head_dim, float scale, int kv_rows, void* stream) {
    if (rows <= 0 || H <= 0 || head_dim != HD || kv_rows < 1 || kv_rows > DECR_MAXS || (ld % 8) || (ldq % 8) || (ldo % 8) || !klen) return SVLA_EINVAL;
    DecRowsArgs p{Q, K, V, ld, O, ldo, LSE, klen, cache_row, H, scale, kv_rows, ldq};
    return SVLA_LAUNCH(attn_decode_rows_kernel, attn_decode_rows_kernel_body, DECR_THREADS, 1, dim3(rows * H), dim3(DECR_THREADS), 0, (hipStream_t)stream, p);
}

// ------------------------------------------------------------------------------------------------
// llama KV-cache append (llama/model.py:279-293: cache[:bsz, start_pos] = xk / xv) with a cache row and a slot PER ROW, both read from device memory:
// cache[cache_row[r], pos[r], :] = src[r, :].  pos[r] < 0: the row is skipped; a slot at or beyond cache_rows, or a negative cache row, writes nothing either.
__device__ __forceinline__ void kv_append_rows_kernel_body(const bf16_t* __restrict__ src, long ld_src, bf16_t* __restrict__ cache, long cache_rows, int width,
                                                           const int* __restrict__ cache_row, const int* __restrict__ pos, int rows) {
    const int cpr = width / 8;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < rows * cpr; i += gridDim.x * blockDim.x) {
        const int r = i / cpr, c = (i % cpr) * 8;
        const int t = pos[r], cr = cache_row ? cache_row[r] : r;
        if (t < 0 || t >= cache_rows || cr < 0) continue;
        *(u32x4*)(cache + ((size_t)cr * cache_rows + t) * width + c) = *(const u32x4*)(src + (size_t)r * ld_src + c);
    }
}
__global__ void kv_append_rows_kernel(const bf16_t* __restrict__ src, long ld_src, bf16_t* __restrict__ cache, long cache_rows, int width,
                                      const int* __restrict__ cache_row, const int* __restrict__ pos, int rows) {
    kv_append_rows_kernel_body(src, ld_src, cache, cache_rows, width, cache_row, pos, rows);
}
extern "C" int svla_kv_append_rows_bf16(const bf16_t* src, long ld_src, bf16_t* cache, long cache_rows, int width, const int* cache_row, const int* pos, int rows,
                                        void* stream) {
    if (rows <= 0 || width <= 0 || (width % 8) || (ld_src % 8) || cache_rows <= 0 || !pos) return SVLA_EINVAL;
    int blocks = (rows * (width / 8) + 255) / 256; if (blocks > 1024) blocks = 1024;
    return SVLA_LAUNCH(kv_append_rows_kernel, kv_append_rows_kernel_body, 1024, 1, dim3(blocks), dim3(256), 0, (hipStream_t)stream, src, ld_src, cache, cache_rows, width,
                       cache_row, pos, rows);
}
