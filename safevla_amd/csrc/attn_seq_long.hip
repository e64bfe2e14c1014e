// Causal attention forward over whole episodes (include/svla.h: svla_attn_causal_fwd_bf16), bf16 in / out, fp32 scores, softmax and accumulators, head_dim 64,
// 1 <= S <= 1024 keys (gfx950, v_mfma_f32_16x16x32_bf16).  The tile kernels of attn.hip keep K and V of a whole (row, head) in LDS and a query tile's full score row in
// registers: at S = 1024 that is 256 KiB of LDS.  Here K and V are STREAMED: a workgroup of four waves owns one tile of CSL_QT = 64 queries of one (row, head) (16 per
// wave) and walks the 64-key tiles at or below its diagonal, two LDS buffers of one K tile + one V tile each (32 KiB + 4 KiB of trajectory ids: four workgroups per
// CU), the next tile's global loads in flight under the current tile's MFMAs, ONE barrier per tile.  The softmax is online: a running maximum and a running sum per
// query, the accumulators rescaled when the maximum moves.
//
// Arithmetic of the block-causal form of attn_fwd_kernel_body (csrc/attn.hip; llama/model.py:249-322 with the traj_index mask of allenact_dino_transformer.py:398-402):
// swapped S^T = K.Q^T so that a query's scores are lane-local, scores in the log2 domain, probabilities rounded to bf16 as the A operand of P.V, the denominator
// summed in fp32 from the unrounded values, LSE as a natural log.  What differs is the online rescale, so the two families agree to rounding, not bit for bit.
// Query i sees keys j <= i with traj[j] == traj[i] (traj == NULL: every j <= i); it always sees itself, so no row is empty.
//
// Work order: query tile qt walks qt + 1 key tiles, so the late tiles are the long ones.  blockIdx.y = 0 is the LAST query tile: the dispatcher hands out
// workgroups in x-then-y order, the heavy tiles start first and the short ones fill the tail.
#include "attn_host.h"      // AttnCall / AttnLimits / attn_accepts; attn_common.h: swizzle, row bases, transposed reads

#define HD 64
#define CSL_THREADS 256
#define CSL_QT 64             // queries per workgroup: 16 per wave
#define CSL_KT 64             // keys per tile
#define CSL_MAXS 1024

struct CausalLongArgs {
    const bf16_t *Q, *K, *V; long ld;
    bf16_t* O; long ldo;
    float* LSE;                           // [rows, H, S] or null
    const int* traj;                      // [rows, S] or null
    int S, H;
    float scale;
};

// the 16-byte chunks of one 64-key tile of K and of V that this thread stages: chunk c of rows (tid >> 3) and (tid >> 3) + 32; rows at or beyond S are zeros
struct CslStage { u32x4 k[2], v[2]; };
__device__ __forceinline__ CslStage csl_load(const bf16_t* Kh, const bf16_t* Vh, long ld, int S, int key0, int tid) {
    CslStage s;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int key = key0 + (tid >> 3) + 32 * i;
        const bool ok = key < S;
        const size_t off = (size_t)(ok ? key : 0) * ld + (tid & 7) * 8;
        s.k[i] = ok ? *(const u32x4*)(Kh + off) : u32x4{0, 0, 0, 0};
        s.v[i] = ok ? *(const u32x4*)(Vh + off) : u32x4{0, 0, 0, 0};
    }
    return s;
}
__device__ __forceinline__ void csl_store(bf16_t* Ks, bf16_t* Vs, const CslStage& s, int tid) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = (tid >> 3) + 32 * i;
        const int off = row * LDSROW + (((tid & 7) ^ att_swz(row)) << 3);
        *(u32x4*)(Ks + off) = s.k[i];
        *(u32x4*)(Vs + off) = s.v[i];
    }
}

__device__ __forceinline__ void attn_causal_long_kernel_body(CausalLongArgs p) {
    __shared__ __attribute__((aligned(16))) bf16_t Kbuf[2][CSL_KT * LDSROW];
    __shared__ __attribute__((aligned(16))) bf16_t Vbuf[2][CSL_KT * LDSROW];
    __shared__ __attribute__((aligned(16))) int traj_s[CSL_MAXS];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int ql = lane & 15, g = lane >> 4;
    const int S = p.S;
    const int r = blockIdx.x / p.H, h = blockIdx.x % p.H;
    const int qt = (int)gridDim.y - 1 - (int)blockIdx.y;      // heavy tiles first
    const size_t tok0 = (size_t)r * S;
    const bf16_t* Kh = p.K + tok0 * p.ld + h * HD;
    const bf16_t* Vh = p.V + tok0 * p.ld + h * HD;
    const bool has_traj = p.traj != nullptr;

    CslStage st = csl_load(Kh, Vh, p.ld, S, 0, tid);
    // this lane's query: row ql of the wave's 16-query tile, dims 8g .. 8g+7 and 32 + 8g .. (the B operand of S^T = K.Q^T)
    const int q = qt * CSL_QT + wid * 16 + ql;
    bf16x8 qf[2];
    {
        const bool ok = q < S;
        const bf16_t* qp = p.Q + (tok0 + (ok ? q : 0)) * p.ld + h * HD + 8 * g;
        qf[0] = gld8(qp, ok);
        qf[1] = gld8(qp + 32, ok);
    }
    if (has_traj) {      // ids of the keys this tile can see (and of its own queries); beyond S: -1
        for (int i = tid; i < (qt + 1) * CSL_KT; i += CSL_THREADS) traj_s[i] = i < S ? p.traj[tok0 + i] : -1;
    }
    const float sl2 = p.scale * LOG2E;      // scores in the log2 domain: p = exp2(s * scale * log2e - max)
    float mx = -INFINITY, lsum = 0.f;       // running maximum of the query's row; this LANE's share of the running sum (keys 4g .. 4g+3 of every 16)
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    int tq = 0;

    for (int j = 0; j <= qt; ++j) {
        bf16_t* Ks = Kbuf[j & 1];
        bf16_t* Vs = Vbuf[j & 1];
        // buffer j & 1 was last read by tile j - 2; every wave has passed the barrier of tile j - 1 since
        csl_store(Ks, Vs, st, tid);
        __syncthreads();
        if (j < qt) st = csl_load(Kh, Vh, p.ld, S, (j + 1) * CSL_KT, tid);
        if (has_traj && j == 0) tq = traj_s[q];      // (q < (qt + 1) * 64 <= 1024; staged before the first barrier)
        const RowBase Krow = att_row_base(Ks, lane);
        const TrBase Vtr = att_tr_base(Vs, lane);
        const bool diag = j == qt;
        // on the diagonal tile wave w sees the 16-key sub-tiles 0 .. w only (wave-uniform)
        const int nsub = diag ? wid + 1 : 4;
        float sc[4][4];
        float tmx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            if (kt < nsub) {
                f32x4 a = {0.f, 0.f, 0.f, 0.f};
                a = mfma16(lds_row8i(Krow.lo, kt * 16), qf[0], a);
                a = mfma16(lds_row8i(Krow.hi, kt * 16), qf[1], a);
                const int key0 = j * CSL_KT + kt * 16 + 4 * g;
                int tk[4] = {0, 0, 0, 0};
                if (has_traj) {
                    const int4 t4 = *(const int4*)(traj_s + key0);
                    tk[0] = t4.x; tk[1] = t4.y; tk[2] = t4.z; tk[3] = t4.w;
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float s = a[e] * sl2;
                    if ((diag && key0 + e > q) || (has_traj && tk[e] != tq)) s = -INFINITY;
                    sc[kt][e] = s;
                    tmx = fmaxf(tmx, s);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) sc[kt][e] = -INFINITY;
            }
        }
        tmx = fmaxf(tmx, __shfl_xor(tmx, 16, 64));
        tmx = fmaxf(tmx, __shfl_xor(tmx, 32, 64));
        // online softmax: a tile that is wholly hidden from this query (another trajectory) leaves mx at -inf; exp2 then runs against 0, every p is 0
        const float mnew = fmaxf(mx, tmx);
        const float mref = mnew == -INFINITY ? 0.f : mnew;
        const float alpha = __builtin_amdgcn_exp2f(mx - mref);
        mx = mnew;
        float tsum = 0.f;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int e = 0; e < 4; ++e) { sc[kt][e] = __builtin_amdgcn_exp2f(sc[kt][e] - mref); tsum += sc[kt][e]; }
        lsum = lsum * alpha + tsum;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] *= alpha;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (2 * u < nsub) {
                const float pv[8] = {sc[2 * u][0], sc[2 * u][1], sc[2 * u][2], sc[2 * u][3], sc[2 * u + 1][0], sc[2 * u + 1][1], sc[2 * u + 1][2], sc[2 * u + 1][3]};
                const bf16x8 pa = pack8(pv);
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) o[dt] = mfma16(lds_tr8i(Vtr.d[dt], 32 * u, 32 * u + 16), pa, o[dt]);      // O^T: rows = head dims, cols = queries
            }
        }
    }
    lsum += __shfl_xor(lsum, 16, 64);
    lsum += __shfl_xor(lsum, 32, 64);
    // o[dt][e]: query q, head dim dt*16 + 4g + e
    if (q < S) {
        const float inv = lsum > 0.f ? 1.f / lsum : 0.f;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            const u32x2 w = {pack_bf2(o[dt][0] * inv, o[dt][1] * inv), pack_bf2(o[dt][2] * inv, o[dt][3] * inv)};
            *(u32x2*)(p.O + (tok0 + q) * p.ldo + h * HD + dt * 16 + 4 * g) = w;
        }
        if (p.LSE && g == 0) p.LSE[((size_t)r * p.H + h) * S + q] = (mx + __log2f(lsum)) * LN2;      // natural log, the layout svla_attn_bwd_bf16 reads
    }
}
__global__ void __launch_bounds__(CSL_THREADS, 2) attn_causal_long_kernel(CausalLongArgs p) { attn_causal_long_kernel_body(p); }

extern "C" int svla_attn_causal_fwd_bf16(const bf16_t* Q, const bf16_t* K, const bf16_t* V, long ld, bf16_t* O, long ldo, float* LSE, int rows, int S, int H, int head_dim,
                                         float scale, const int* traj, void* stream) {
    if (head_dim != HD || !Q || !K || !V || !O) return SVLA_EINVAL;
    AttnCall c{};
    c.Q = Q; c.K = K; c.V = V; c.ld = ld; c.O = O; c.ldo = ldo; c.LSE = LSE; c.rows = rows; c.S = S; c.H = H; c.scale = scale;
    c.mask_mode = traj ? MASK_BLOCK_CAUSAL : MASK_NONE;      // the record's mask is the trajectory mask; causality is the family's own
    c.traj = traj; c.stream = (hipStream_t)stream;
    if (!attn_accepts(c, ATTN_FWD_64_CAUSAL_L) || ld < (long)H * HD || ldo < (long)H * HD || (long)rows * H > 0x7fffffffL) return SVLA_EINVAL;
    CausalLongArgs p{Q, K, V, ld, O, ldo, LSE, traj, S, H, scale};
    const int nqt = (S + CSL_QT - 1) / CSL_QT;
    return SVLA_LAUNCH(attn_causal_long_kernel, attn_causal_long_kernel_body, CSL_THREADS, 2, dim3((unsigned)rows * (unsigned)H, nqt), dim3(CSL_THREADS), 0, c.stream, p);
}
