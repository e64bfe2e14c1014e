// Row kernels of the padded-step skip of the imitation-learning model (il.EarlyFusionCnnTransformer(skip_padded_steps=True); contracts in include/svla.h):
//   svla_rows_gather         : dst[r] = idx[r] in [0, src_rows) ? src[idx[r]] : 0 over rows of row_bytes bytes -- valid uint8 frames / features out of the padded
//                              [B * T] batch, compact fusion outputs into decoder-row order, the decoder-input gradient back to compact rows (the inverse table)
//   svla_fusion_text_bwd_seg : the text-feature gradient over compact rows ordered goal by goal: goal u owns the rows seg[u] ... seg[u + 1]
#include "common.h"

#define GATHER_THREADS 256
#define GATHER_UNROLL 4             // 16-byte loads in flight per lane before the first store
#define GATHER_MAX_BLOCKS 2048      // 256 compute units x 8 workgroups: the rest is a grid stride

// One work item = one 16-byte vector of one destination row, numbered row-major over (row, vector): neighbouring lanes read neighbouring vectors of a row whatever
// its length, so 4 rows of 258 048 bytes fill the chip like 16 384 rows of 1 KiB do.  Three passes per trip so that the loads of a pass are independent of each
// other: the GATHER_UNROLL indices (device memory; L1 hits: a wave spans at most two rows of >= 1 KiB), then the GATHER_UNROLL vectors, then the stores.  An index
// outside [0, src_rows) -- the -1 of a padded step, or anything else -- reads nothing and stores zeros.  Vector numbers are 32-bit (the host refuses more).
__global__ void __launch_bounds__(GATHER_THREADS) rows_gather_kernel(u32x4* __restrict__ dst, long dst_vec_stride, const u32x4* __restrict__ src, long src_vec_stride,
                                                                       const int* __restrict__ idx, unsigned total, unsigned vec_per_row, int src_rows) {
    const unsigned step = gridDim.x * GATHER_THREADS;
    for (unsigned v0 = blockIdx.x * GATHER_THREADS + threadIdx.x; v0 < total; v0 += GATHER_UNROLL * step) {      // (total < 2^31, GATHER_UNROLL * step <= 2^21: no wrap)
        unsigned r[GATHER_UNROLL], c[GATHER_UNROLL];
        int s[GATHER_UNROLL];
        u32x4 w[GATHER_UNROLL];
#pragma unroll
        for (int k = 0; k < GATHER_UNROLL; ++k) {
            const unsigned v = v0 + k * step;
            r[k] = v / vec_per_row;
            c[k] = v - r[k] * vec_per_row;
            s[k] = v < total ? idx[r[k]] : -1;
        }
#pragma unroll
        for (int k = 0; k < GATHER_UNROLL; ++k) {
            w[k] = u32x4{0u, 0u, 0u, 0u};
            if (s[k] >= 0 && s[k] < src_rows) w[k] = src[(long)s[k] * src_vec_stride + c[k]];
        }
#pragma unroll
        for (int k = 0; k < GATHER_UNROLL; ++k)
            if (v0 + k * step < total) dst[(long)r[k] * dst_vec_stride + c[k]] = w[k];
    }
}

extern "C" int svla_rows_gather(void* dst, long dst_stride, const void* src, long src_stride, const int* idx, int rows, long row_bytes, int src_rows, void* stream) {
    if (rows <= 0 || src_rows <= 0 || row_bytes <= 0 || (row_bytes % 16) || (dst_stride % 16) || (src_stride % 16) || dst_stride < row_bytes || src_stride < row_bytes ||
        !dst || !src || !idx || ((uintptr_t)dst % 16) || ((uintptr_t)src % 16))
        return SVLA_EINVAL;
    const long vpr = row_bytes / 16, total = (long)rows * vpr;
    if (total >= (1L << 31)) return SVLA_EINVAL;      // 32 GiB of destination rows: the kernel numbers vectors in 32 bits
    long blocks = (total + GATHER_THREADS * GATHER_UNROLL - 1) / (GATHER_THREADS * GATHER_UNROLL);
    if (blocks > GATHER_MAX_BLOCKS) blocks = GATHER_MAX_BLOCKS;
    return svla_launch<rows_gather_kernel>(dim3((unsigned)blocks), dim3(GATHER_THREADS), 0, (hipStream_t)stream, (u32x4*)dst, dst_stride / 16, (const u32x4*)src,
                                           src_stride / 16, idx, (unsigned)total, (unsigned)vpr, src_rows);
}

// dtext[u, j, :] = sum over the rows r in [seg[u], seg[u + 1]) of dx0[r, text_off + j, :].  The segmented form of fusion_text_bwd_kernel (misc.hip), which walks a
// goal's rows as the column b of a [T, B] grid: here the rows of a goal are contiguous, one workgroup (one wave) per (goal, text token, 512-wide slice) walks them
// and owns its 8 destination floats per lane -- a plain store, no atomics, so the result does not depend on the launch; a goal without rows gets zeros.
__global__ void __launch_bounds__(64) fusion_text_bwd_seg_kernel(const bf16_t* __restrict__ dx0, const int* __restrict__ seg, int S, int L, int text_off, int D,
                                                                 float* __restrict__ dtext) {
    const int u = blockIdx.x, j = blockIdx.y, lane = threadIdx.x;
    const int c = blockIdx.z * 512 + lane * 8;
    if (c >= D) return;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int r0 = seg[u], r1 = seg[u + 1];
    const bf16_t* p = dx0 + ((size_t)r0 * S + text_off + j) * D + c;
#pragma unroll 4
    for (int r = r0; r < r1; ++r, p += (size_t)S * D) {
        const u32x4 w = *(const u32x4*)p;
#pragma unroll
        for (int e = 0; e < 4; ++e) { acc[2 * e] += bf_lo(w[e]); acc[2 * e + 1] += bf_hi(w[e]); }
    }
    float* d = dtext + ((size_t)u * L + j) * D + c;
    *(f32x4*)d = f32x4{acc[0], acc[1], acc[2], acc[3]};
    *(f32x4*)(d + 4) = f32x4{acc[4], acc[5], acc[6], acc[7]};
}

extern "C" int svla_fusion_text_bwd_seg(const bf16_t* dx0, const int* seg, int U, int S, int L, int text_off, int D, float* dtext, void* stream) {
    if (U <= 0 || L <= 0 || text_off < 0 || text_off + L > S || D <= 0 || (D % 8) || !dx0 || !seg || !dtext) return SVLA_EINVAL;
    return svla_launch<fusion_text_bwd_seg_kernel>(dim3(U, L, (D + 511) / 512), dim3(64), 0, (hipStream_t)stream, dx0, seg, S, L, text_off, D, dtext);
}
