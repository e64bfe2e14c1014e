// Single-query ("decode") attention forward, bf16, head_dim 64: the KV-cached acting step of the llama decoder (one new token per env against a cache window;
// allenact_dino_transformer.py:388-397; the reference's caches and both policies are built for max_length = 1000) and the pruned last fusion layer in eval mode.
// The tile kernels of attn.hip stage all S keys of K and V into LDS for that one query (128 KiB and 73 us per launch at S = 500, whatever the window); the three
// kernels here read ONLY the valid keys, straight from global memory.
//
// The family's contract, stated once.  One query per row, no bias / trajectory mask / dropout; Q [rows, ldq], K / V [cache rows x kv_rows, ld], O [rows, ldo],
// optional LSE [rows, H] (natural log).  Arithmetic of the MFMA path: bf16 products, fp32 accumulation, probabilities rounded to bf16 before the product with V.
// A row without a valid key yields zeros and a non-finite LSE.  One workgroup of DEC_THREADS = 256 threads per (row, head); thread (g = tid / 8, c = tid % 8)
// owns the 16-byte chunk c of key 32 b + g of block b.  Pass 1: a key's score is reduced over its eight lanes, the maximum over the workgroup.  Pass 2: exp2 and
// P.V in ascending block order per thread, then sums over the 32 key groups (lanes, then the four waves through LDS).  These steps are the dec_* helpers below and
// every kernel calls the same ones (but for one dec_pv that the long kernel writes out, see there), so the three round and sum alike: the same keys give the same
// bits (tests/test_attn_decode_rows_gpu.py).
//
// What a kernel body holds is only what differs: how it enumerates blocks, how it decides that a key is valid, how it issues its K and V loads.
//   attn_decode_kernel        svla_attn_fwd_bf16, S <= 512.  Keys: kvalid [rows, S] bytes or null (all of S), kv_rows >= S.  16 unrolled blocks with loads under the
//                             lanes' own condition; the scores wait between the passes in 16 registers.
//   attn_decode_long_kernel   svla_attn_fwd_bf16, 512 < S <= DEC_MAXS.  Same key set.  32 scores in registers next to the loads in flight would not fit, and on
//                             the recorded acting path S is the whole cache window at every step while only [max(t - time_step, 0), t] is valid.  So the row's
//                             kvalid bytes are read ONCE (4 keys per thread) into LDS, a ballot turns them into a 32-bit mask of the blocks that hold a valid key,
//                             and both passes walk only the set bits, DEC_U blocks per trip with all of a trip's loads issued before the first use: the cost
//                             follows the episode's length, not the window.  The scores wait in LDS (4 KiB).
//   attn_decode_rows_kernel   svla_attn_decode_rows_bf16: every row is an episode of its own (a vector of evaluation episodes that start, end and stall
//                             independently, one set of weights, one call per layer whose arguments do not depend on the step).  Keys: the prefix
//                             [0, min(klen[r], kv_rows)) of cache row cache_row[r] (null: r), both read from device memory; no validity bytes and no ballot, the
//                             block count comes from klen and only the last block is partial: a counted walk, DEC_U blocks per trip, scores in LDS.  The cost
//                             follows klen[r], not kv_rows.  Its V loads are unconditional and selected afterwards (see there).
// kv_append_rows_kernel (below the attention kernels) writes the rings that the rows kernel reads.
#include "attn_host.h"      // AttnCall, DEC_MAXS; attn_common.h: LOG2E / LN2; common.h: bf16 helpers, SVLA_LAUNCH

#define HD 64
#define DEC_THREADS 256
#define DEC_MAXB 16          // attn_decode_kernel: 16 blocks of 32 keys (S <= 512)
#define DEC_U 8              // the LDS-score kernels: blocks per trip, 8 x 16 bytes per thread in flight

struct DecArgs {
    const bf16_t *Q, *K, *V; long ld;
    bf16_t* O; long ldo;
    float* LSE;                           // [rows, H] or null
    const unsigned char* kvalid;          // [rows, S] or null                 (the two kernels behind svla_attn_fwd_bf16)
    const int* klen;                      // [rows]                            (the rows kernel)
    const int* cache_row;                 // [rows] or null: identity          (the rows kernel)
    int S, H;                             // S: with kvalid only
    float scale;
    int kv_rows;
    long ldq;
};
struct DecShared {                        // the workgroup reductions: [wave][0] maximum, [wave][1] sum; the waves' P.V partial sums
    float red[4][2];
    alignas(16) float accs[4][64];        // (16-byte stores of a lane's eight sums)
};

// ---- the steps every kernel shares: query load, a key's score (dot, then reduce), workgroup maximum, one key's P.V step, the epilogue
// chunk c of head h of row `row` of a [*, ld] matrix
__device__ __forceinline__ bf16x8 dec_ld8(const bf16_t* base, size_t row, long ld, int h, int c) { return *(const bf16x8*)(base + row * ld + h * HD + c * 8); }

__device__ __forceinline__ void dec_load_q(const DecArgs& p, int r, int h, int c, float (&qv)[8]) {
    const bf16x8 q8 = dec_ld8(p.Q, (size_t)r, p.ldq, h, c);
#pragma unroll
    for (int e = 0; e < 8; ++e) qv[e] = bf2f((bf16_t)q8[e]);
}
// this lane's eighth of a key's dot product with the query
__device__ __forceinline__ float dec_dot(const float (&qv)[8], bf16x8 k8) {
    float d = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) d = fmaf(qv[e], bf2f((bf16_t)k8[e]), d);
    return d;
}
// a key's scaled score (log2 domain) from the eight partial dot products that its eight lanes hold; -inf when !ok (ok is uniform over them)
__device__ __forceinline__ float dec_score(float d, bool ok, float sl2) {
    d += __shfl_xor(d, 1, 64); d += __shfl_xor(d, 2, 64); d += __shfl_xor(d, 4, 64);
    return ok ? d * sl2 : -INFINITY;
}
// maximum over the workgroup of the threads' running maxima; 0 for a row without a key.  Its barrier also publishes the scores that pass 1 wrote to LDS.
__device__ __forceinline__ float dec_wg_max(float mx, DecShared& sh, int lane, int wid) {
    mx = fmaxf(mx, __shfl_xor(mx, 8, 64)); mx = fmaxf(mx, __shfl_xor(mx, 16, 64)); mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    if (lane == 0) sh.red[wid][0] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(sh.red[0][0], sh.red[1][0]), fmaxf(sh.red[2][0], sh.red[3][0]));
    return mx == -INFINITY ? 0.f : mx;
}
// one key's P.V step: adds its share to acc and returns its probability for the thread's sum
__device__ __forceinline__ float dec_pv(float s, float mx, bf16x8 v8, float (&acc)[8]) {
    const float pr = __builtin_amdgcn_exp2f(s - mx);
    const float pb = bf2f(f2bf(pr));                         // the MFMA path's operand rounding
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = fmaf(pb, bf2f((bf16_t)v8[e]), acc[e]);
    return pr;
}
// sums over the key groups, normalise, store O and LSE
__device__ __forceinline__ void dec_finish(const DecArgs& p, int r, int h, float mx, const float (&acc)[8], float lsum, DecShared& sh) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    // every key was counted by its eight lanes: sum over lanes / 8; the accumulators: over the lanes that share chunk c
    lsum += __shfl_xor(lsum, 1, 64); lsum += __shfl_xor(lsum, 2, 64); lsum += __shfl_xor(lsum, 4, 64);
    lsum += __shfl_xor(lsum, 8, 64); lsum += __shfl_xor(lsum, 16, 64); lsum += __shfl_xor(lsum, 32, 64);
    float a[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        a[e] = acc[e];
        a[e] += __shfl_xor(a[e], 8, 64); a[e] += __shfl_xor(a[e], 16, 64); a[e] += __shfl_xor(a[e], 32, 64);
    }
    if (lane == 0) sh.red[wid][1] = lsum * 0.125f;
    if (lane < 8) {
#pragma unroll
        for (int e = 0; e < 8; ++e) sh.accs[wid][lane * 8 + e] = a[e];
    }
    __syncthreads();
    if (tid < 64) {
        const float ls = (sh.red[0][1] + sh.red[1][1]) + (sh.red[2][1] + sh.red[3][1]);
        const float o = (sh.accs[0][tid] + sh.accs[1][tid]) + (sh.accs[2][tid] + sh.accs[3][tid]);
        const float inv = ls > 0.f ? 1.f / ls : 0.f;
        p.O[(size_t)r * p.ldo + h * HD + tid] = f2bf(o * inv);
        if (p.LSE && tid == 0) p.LSE[(size_t)r * p.H + h] = (mx + __log2f(ls)) * LN2;
    }
}

// ------------------------------------------------------------------------------------------------ S <= 512: 16 unrolled blocks, scores in registers
__device__ __forceinline__ void attn_decode_kernel_body(DecArgs p) {
    __shared__ DecShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int g = tid >> 3, c = tid & 7;
    const int r = blockIdx.x / p.H, h = blockIdx.x % p.H;
    const int S = p.S;
    const size_t tok0 = (size_t)r * p.kv_rows;
    const unsigned char* kvr = p.kvalid ? p.kvalid + (size_t)r * S : nullptr;
    const float sl2 = p.scale * LOG2E;
    float qv[8];
    dec_load_q(p, r, h, c, qv);
    const int nb = (S + 31) >> 5;
    float sc[DEC_MAXB];
    unsigned vmask = 0;
    float mx = -INFINITY;
#pragma unroll
    for (int b = 0; b < DEC_MAXB; ++b) {
        sc[b] = -INFINITY;
        if (b < nb) {
            const int key = b * 32 + g;
            const bool ok = key < S && (!kvr || kvr[key]);
            float d = 0.f;
            if (ok) {
                d = dec_dot(qv, dec_ld8(p.K, tok0 + key, p.ld, h, c));
                vmask |= 1u << b;
            }
            sc[b] = dec_score(d, ok, sl2);
            mx = fmaxf(mx, sc[b]);
        }
    }
    mx = dec_wg_max(mx, sh, lane, wid);
    float acc[8], lsum = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll
    for (int b = 0; b < DEC_MAXB; ++b) {
        if (b < nb && ((vmask >> b) & 1u)) lsum += dec_pv(sc[b], mx, dec_ld8(p.V, tok0 + b * 32 + g, p.ld, h, c), acc);
    }
    dec_finish(p, r, h, mx, acc, lsum, sh);
}
__global__ void __launch_bounds__(DEC_THREADS) attn_decode_kernel(DecArgs p) { attn_decode_kernel_body(p); }

// ------------------------------------------------------------------------------------------------ 512 < S <= DEC_MAXS: the set-bit walk, scores in LDS
__device__ __forceinline__ void attn_decode_long_kernel_body(DecArgs p) {
    __shared__ unsigned vs4[DEC_MAXS / 4];      // one validity byte per key (0: masked, or beyond S)
    __shared__ float ps[DEC_MAXS];              // scaled scores (log2 domain) of the keys of the valid blocks; -inf: masked
    __shared__ unsigned wbits[4];
    __shared__ DecShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int g = tid >> 3, c = tid & 7;
    const int r = blockIdx.x / p.H, h = blockIdx.x % p.H;
    const int S = p.S;
    const size_t tok0 = (size_t)r * p.kv_rows;
    const float sl2 = p.scale * LOG2E;
    // ---- validity: thread tid looks at keys 4 tid .. 4 tid + 3, so block b (32 keys) is lanes 8 b' .. 8 b' + 7 of wave b / 8
    {
        const unsigned char* kvr = p.kvalid ? p.kvalid + (size_t)r * S : nullptr;
        unsigned w = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int key = tid * 4 + j;
            const bool ok = key < S && (!kvr || kvr[key]);
            w |= (ok ? 1u : 0u) << (8 * j);
        }
        vs4[tid] = w;
        const unsigned long long bal = __ballot(w != 0);
        if (lane == 0) {
            unsigned m = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) m |= ((bal >> (8 * j)) & 0xffull) ? (1u << j) : 0u;
            wbits[wid] = m;
        }
    }
    float qv[8];
    dec_load_q(p, r, h, c, qv);
    __syncthreads();
    const unsigned char* vs = (const unsigned char*)vs4;
    const unsigned bmask = __builtin_amdgcn_readfirstlane(wbits[0] | (wbits[1] << 8) | (wbits[2] << 16) | (wbits[3] << 24));
    // ---- pass 1: scores of the valid blocks -> LDS, running maximum
    float mx = -INFINITY;
    for (unsigned m = bmask; m;) {
        int key[DEC_U];
        bool ok[DEC_U];
        bf16x8 k8[DEC_U];
#pragma unroll
        for (int u = 0; u < DEC_U; ++u) {
            key[u] = m ? __builtin_ctz(m) * 32 + g : -1;      // (m is wave-uniform)
            m &= m - 1;
            ok[u] = key[u] >= 0 && vs[key[u]];
            k8[u] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
            if (ok[u]) k8[u] = dec_ld8(p.K, tok0 + key[u], p.ld, h, c);
        }
#pragma unroll
        for (int u = 0; u < DEC_U; ++u) {
            if (key[u] >= 0) {
                const float s = dec_score(dec_dot(qv, k8[u]), ok[u], sl2);
                if (c == 0) ps[key[u]] = s;
                mx = fmaxf(mx, s);
            }
        }
    }
    mx = dec_wg_max(mx, sh, lane, wid);
    // ---- pass 2: probabilities and P.V over the same blocks
    float acc[8], lsum = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    for (unsigned m = bmask; m;) {
        float s[DEC_U];
        bf16x8 v8[DEC_U];
#pragma unroll
        for (int u = 0; u < DEC_U; ++u) {
            const int key = m ? __builtin_ctz(m) * 32 + g : -1;
            m &= m - 1;
            s[u] = key >= 0 ? ps[key] : -INFINITY;
            v8[u] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
            if (s[u] != -INFINITY) v8[u] = dec_ld8(p.V, tok0 + key, p.ld, h, c);
        }
#pragma unroll
        for (int u = 0; u < DEC_U; ++u) {
            // dec_pv, written out: under these per-lane conditions the compiler carries the helper's acc through the trip as one 8-wide value instead of four
            // pairs, and the kernel takes 102 VGPRs instead of 73 (tests/test_attn_decode_resources_cpu.py)
            if (s[u] != -INFINITY) {
                const float pr = __builtin_amdgcn_exp2f(s[u] - mx);
                lsum += pr;
                const float pb = bf2f(f2bf(pr));
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] = fmaf(pb, bf2f((bf16_t)v8[u][e]), acc[e]);
            }
        }
    }
    dec_finish(p, r, h, mx, acc, lsum, sh);
}
__global__ void __launch_bounds__(DEC_THREADS) attn_decode_long_kernel(DecArgs p) { attn_decode_long_kernel_body(p); }

// ------------------------------------------------------------------------------------------------ per-row KV rings: the counted walk, scores in LDS
__device__ __forceinline__ void attn_decode_rows_kernel_body(DecArgs p) {
    __shared__ float ps[DEC_MAXS];              // scaled scores (log2 domain) of the keys of the blocks in use; -inf: beyond the row's length
    __shared__ DecShared sh;
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
    dec_load_q(p, r, h, c, qv);
    // ---- pass 1: scores of blocks [0, nb) -> LDS, running maximum
    float mx = -INFINITY;
    for (int b0 = 0; b0 < nb; b0 += DEC_U) {
        bool ok[DEC_U];
        bf16x8 k8[DEC_U];
#pragma unroll
        for (int u = 0; u < DEC_U; ++u) {
            const int key = (b0 + u) * 32 + g;
            ok[u] = key < n;                                  // (false for every block at or beyond nb)
            k8[u] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
            if (ok[u]) k8[u] = dec_ld8(p.K, tok0 + key, p.ld, h, c);
        }
#pragma unroll
        for (int u = 0; u < DEC_U; ++u) {
            if (b0 + u < nb) {                                // wave-uniform
                const float s = dec_score(dec_dot(qv, k8[u]), ok[u], sl2);
                if (c == 0) ps[(b0 + u) * 32 + g] = s;
                mx = fmaxf(mx, s);
            }
        }
    }
    mx = dec_wg_max(mx, sh, lane, wid);
    // ---- pass 2: probabilities and P.V over the same blocks
    float acc[8], lsum = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    for (int b0 = 0; b0 < nb; b0 += DEC_U) {
        float s[DEC_U];
        bf16x8 v8[DEC_U];
#pragma unroll
        for (int u = 0; u < DEC_U; ++u) {
            const int key = (b0 + u) * 32 + g;
            s[u] = b0 + u < nb ? ps[key] : -INFINITY;
            // every lane loads, a key beyond n from key 0 of the row (n >= 1 inside this loop; the line is in cache), and the value is dropped by a select: with a
            // load under the lanes' own condition the compiler moves the bf16 unpacking up into each load's branch and waits for every load by itself
            // (profiles/vector_agent_ab.txt: 36.97 against 26.93 us per launch)
            const bf16x8 ld8 = dec_ld8(p.V, tok0 + (key < n ? key : 0), p.ld, h, c);
            v8[u] = key < n ? ld8 : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        }
#pragma unroll
        for (int u = 0; u < DEC_U; ++u) {
            if (b0 + u < nb) lsum += dec_pv(s[u], mx, v8[u], acc);      // wave-uniform; a key beyond n has s = -inf and v = 0 and adds exactly nothing
        }
    }
    dec_finish(p, r, h, mx, acc, lsum, sh);
}
__global__ void __launch_bounds__(DEC_THREADS) attn_decode_rows_kernel(DecArgs p) { attn_decode_rows_kernel_body(p); }

// ------------------------------------------------------------------------------------------------ launchers
// One query per row behind svla_attn_fwd_bf16 (attn.hip routes here): 1 <= S <= DEC_MAXS
int attn_decode_launch(const AttnCall& c) {
    if (!attn_accepts(c, ATTN_FWD_64_DECODE)) return SVLA_EINVAL;
    const long ldq = c.Sq > 0 ? c.ldq : c.ld;      // (Sq == 0 with S == 1 is one query too: on the K/V stride)
    DecArgs p{c.Q, c.K, c.V, c.ld, c.O, c.ldo, c.LSE, c.kvalid, nullptr, nullptr, c.S, c.H, c.scale, attn_kv_rows(c), ldq};
    if (c.S <= DEC_MAXB * 32) return SVLA_LAUNCH(attn_decode_kernel, attn_decode_kernel_body, DEC_THREADS, 1, dim3(c.rows * c.H), dim3(DEC_THREADS), 0, c.stream, p);
    return SVLA_LAUNCH(attn_decode_long_kernel, attn_decode_long_kernel_body, DEC_THREADS, 1, dim3(c.rows * c.H), dim3(DEC_THREADS), 0, c.stream, p);
}

extern "C" int svla_attn_decode_rows_bf16(const bf16_t* Q, long ldq, const bf16_t* K, const bf16_t* V, long ld, bf16_t* O, long ldo, float* LSE, const int* klen,
                                          const int* cache_row, int rows, int H, int head_dim, float scale, int kv_rows, void* stream) {
    if (rows <= 0 || H <= 0 || head_dim != HD || kv_rows < 1 || kv_rows > DEC_MAXS || (ld % 8) || (ldq % 8) || (ldo % 8) || !klen) return SVLA_EINVAL;
    DecArgs p{Q, K, V, ld, O, ldo, LSE, nullptr, klen, cache_row, 0, H, scale, kv_rows, ldq};
    return SVLA_LAUNCH(attn_decode_rows_kernel, attn_decode_rows_kernel_body, DEC_THREADS, 1, dim3(rows * H), dim3(DEC_THREADS), 0, (hipStream_t)stream, p);
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
