// Single-query ("decode") attention forward for 512 < S <= 1024, bf16, head_dim 64: the KV-cached acting step of the llama decoder on episodes of up to 1000
// steps (the reference's online evaluation: 600 steps, 1000 for RoomVisit / ObjectNavMulti; its caches and both policies are built for max_length = 1000).
//
// Contract of attn_decode_kernel (csrc/attn.hip): Sq == 1, no bias / trajectory mask / dropout, kvalid [rows, S] or null, kv_rows >= S, ldq, optional LSE
// (natural log); a row without a valid key yields zeros; only valid keys are read from global memory.  Same arithmetic: bf16 products, fp32 accumulation,
// probabilities rounded to bf16 before the product with V.
//
// One workgroup of 256 threads per (row, head), thread (g = tid / 8, c = tid % 8) owns the 16-byte chunk c of key 32 b + g of block b, as there.  What differs:
// that kernel keeps one score per block in registers (16 unrolled blocks); 32 of them plus the loads in flight would not fit, and on the recorded acting path
// S is the whole cache window at every step while only [max(t - time_step, 0), t] is valid.  So here
//  * the row's kvalid bytes are read ONCE (4 keys per thread) into LDS, and a ballot turns them into a 32-bit mask of the blocks that hold a valid key;
//  * both passes walk only the set bits of that mask, DECL_U blocks per trip with all of a trip's loads issued before the first use: the cost follows the
//    episode's length, not the window;
//  * scores wait in LDS (4 KiB) between the passes instead of in registers.
#include "attn_host.h"      // AttnCall, DECL_MAXS; attn_common.h: LOG2E / LN2

#define HD 64
#define DECL_THREADS 256
#define DECL_U 8             // blocks per trip: 8 x 16 bytes per thread in flight

struct DecLongArgs {
    const bf16_t *Q, *K, *V; long ld;
    bf16_t* O; long ldo;
    float* LSE;                           // [rows, H] or null
    const unsigned char* kvalid;          // [rows, S] or null
    int S, H;
    float scale;
    int kv_rows;
    long ldq;
};

__device__ __forceinline__ void attn_decode_long_kernel_body(DecLongArgs p) {
    __shared__ unsigned vs4[DECL_MAXS / 4];      // one validity byte per key (0: masked, or beyond S)
    __shared__ float ps[DECL_MAXS];              // scaled scores (log2 domain) of the keys of the valid blocks; -inf: masked
    __shared__ unsigned wbits[4];
    __shared__ float red[4][2];
    __shared__ float accs[4][64];
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
    {
        const bf16x8 q8 = *(const bf16x8*)(p.Q + (size_t)r * p.ldq + h * HD + c * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) qv[e] = bf2f((bf16_t)q8[e]);
    }
    __syncthreads();
    const unsigned char* vs = (const unsigned char*)vs4;
    const unsigned bmask = __builtin_amdgcn_readfirstlane(wbits[0] | (wbits[1] << 8) | (wbits[2] << 16) | (wbits[3] << 24));
    // ---- pass 1: scores of the valid blocks -> LDS, running maximum
    float mx = -INFINITY;
    for (unsigned m = bmask; m;) {
        int key[DECL_U];
        bool ok[DECL_U];
        bf16x8 k8[DECL_U];
#pragma unroll
        for (int u = 0; u < DECL_U; ++u) {
            key[u] = m ? __builtin_ctz(m) * 32 + g : -1;      // (m is wave-uniform)
            m &= m - 1;
            ok[u] = key[u] >= 0 && vs[key[u]];
            k8[u] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
            if (ok[u]) k8[u] = *(const bf16x8*)(p.K + (tok0 + key[u]) * p.ld + h * HD + c * 8);
        }
#pragma unroll
        for (int u = 0; u < DECL_U; ++u) {
            if (key[u] >= 0) {
                float d = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) d = fmaf(qv[e], bf2f((bf16_t)k8[u][e]), d);
                // the eight lanes of a key hold its eight partial dot products (ok is uniform over them)
                d += __shfl_xor(d, 1, 64); d += __shfl_xor(d, 2, 64); d += __shfl_xor(d, 4, 64);
                const float s = ok[u] ? d * sl2 : -INFINITY;
                if (c == 0) ps[key[u]] = s;
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
    for (unsigned m = bmask; m;) {
        float s[DECL_U];
        bf16x8 v8[DECL_U];
#pragma unroll
        for (int u = 0; u < DECL_U; ++u) {
            const int key = m ? __builtin_ctz(m) * 32 + g : -1;
            m &= m - 1;
            s[u] = key >= 0 ? ps[key] : -INFINITY;
            v8[u] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
            if (s[u] != -INFINITY) v8[u] = *(const bf16x8*)(p.V + (tok0 + key) * p.ld + h * HD + c * 8);
        }
#pragma unroll
        for (int u = 0; u < DECL_U; ++u) {
            if (s[u] != -INFINITY) {
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
__global__ void __launch_bounds__(DECL_THREADS) attn_decode_long_kernel(DecLongArgs p) { attn_decode_long_kernel_body(p); }

int attn_decode_long_launch(const AttnCall& c) {
    if (!attn_accepts(c, ATTN_FWD_64_DECODE_L)) return SVLA_EINVAL;
    DecLongArgs p{c.Q, c.K, c.V, c.ld, c.O, c.ldo, c.LSE, c.kvalid, c.S, c.H, c.scale, attn_kv_rows(c), c.ldq};
    return SVLA_LAUNCH(attn_decode_long_kernel, attn_decode_long_kernel_body, DECL_THREADS, 1, dim3(c.rows * c.H), dim3(DECL_THREADS), 0, c.stream, p);
}
