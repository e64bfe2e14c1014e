// Attention backward for head_dim 64 and 256 < S <= 512, bf16 in/out, fp32 scores / softmax / accumulators (gfx950, v_mfma_f32_16x16x32_bf16).
// The llama decoder attends over the time axis of a rollout or of a whole episode (block-causal on the trajectory ids, key padding, dropout); the
// forward (attn.hip: launch_fwd<18|28|32>) and the KV cache of the acting path already reach 512 steps, this file is the training half.
//
// Same arithmetic contract as the S <= 256 kernel pair of attn.hip (whose header describes the swapped QK^T layout; the LDS swizzle: attn_common.h): P is recomputed
// from the saved natural-log LSE, D = rowsum(dO * O), probabilities and dS are rounded to bf16 before the second product, the dropout element index is
// ((r*H + h)*S + q) * SP4 + k (include/svla.h: svla_dropout), dQ / dK / dV are bf16 and written once each by plain stores (no atomics: bitwise repeatable).
//   dQ    kernel: waves own query tiles, K and V resident in LDS:   dQ = dS.K
//   dK/dV kernel: waves own key tiles,   Q and dO resident in LDS:  dK = dS^T.Q, dV = P^T.dO
// What differs from attn.hip's pair:
//   * two [S, 64] operands are 64 .. 128 KiB of LDS, i.e. ONE workgroup per CU whatever the code does, so a workgroup is EIGHT waves (two per SIMD hide each
//     other's LDS / MFMA latency; the forward measured 1.5x from the same step at S = 433) and a wave may use up to 256 registers;
//   * the loops over a wave's tiles and over the key / query tile pairs are runtime loops on the padded length SP = S rounded up to 32 (one code object per
//     kernel for the whole range instead of one fully unrolled body per 16-key bucket: the unrolled S <= 256 bodies are 6 000 .. 9 000 instructions each);
//   * with the block-causal mask the tile pairs that lie wholly above the diagonal are skipped (wave-uniform loop bounds): half the work of a decoder layer;
//   * the next tile's Q / dO (K / V) fragments are fetched from global memory while the current tile is computed.
// Not built here: the T5 bias (the only biased attention is frozen and has no backward), S > 512, head_dim 96.
#include "attn_host.h"      // AttnCall; attn_common.h: dropout index, LDS swizzle (att_swz) and lane bases, fragment helpers

#define AL_HD 64
#define AL_ROW LDSROW       // LDS row = 128 B, 16-byte chunks XOR-swizzled (att_swz)
#define AL_NW 8
#define AL_THREADS (AL_NW * 64)

struct AttnLongArgs {
    const bf16_t *Q, *K, *V; long ld;     // token row stride (elements) of the k/v tensors
    const bf16_t* O; long ldo;
    const float* LSE;                     // [rows, H, Sq]
    const bf16_t* dO; long lddo;
    bf16_t *dQ, *dK, *dV; long ldd;
    const int* traj;                      // [rows, S] (block-causal)
    const unsigned char* kvalid;          // [rows, S] key padding mask or null
    int S, H, mask_mode;
    float scale;
    int Sq;                               // query rows per batch row present in Q / O / dO / dQ / LSE
    long ldq, lddq;
    DropCfg drop;
};

// stage an [nrows, 64] head slice into SP LDS rows (zero-filled from nrows on): four 16-byte loads per thread in flight before the first LDS store
__device__ __forceinline__ void al_stage(bf16_t* dst, const bf16_t* src, long ld, int nrows, int SP, int tid) {
    const int nchunk = SP * 8;
    for (int q0 = tid; q0 < nchunk; q0 += 4 * AL_THREADS) {
        u32x4 w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = (q0 + i * AL_THREADS) >> 3, c = (q0 + i * AL_THREADS) & 7;
            w[i] = u32x4{0, 0, 0, 0};
            if (row < nrows) w[i] = *(const u32x4*)(src + (size_t)row * ld + c * 8);      // nrows <= SP
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = q0 + i * AL_THREADS, row = q >> 3;
            if (q < nchunk) *(u32x4*)(dst + row * AL_ROW + (((q & 7) ^ att_swz(row)) << 3)) = w[i];
        }
    }
}

// LDS bytes of a kernel at padded length SP: two [SP, 64] bf16 operands + trajectory ids + key mask (+ LSE and D in the dK/dV kernel)
static inline size_t al_lds_dq(int SP) { return (size_t)2 * SP * AL_ROW * sizeof(bf16_t) + (size_t)SP * (sizeof(int) + 1); }
static inline size_t al_lds_dkv(int SP) { return al_lds_dq(SP) + (size_t)SP * 2 * sizeof(float); }

// ================================================================================================ dQ
// MASKED = false: no trajectory mask, no key padding: padded keys have zero K / V rows in LDS (their dS never reaches dQ), padded queries are never stored.
struct AlQFrag { bf16x8 q0, q1, g0, g1; float d, lse; };

template <bool MASKED>
__global__ void __launch_bounds__(AL_THREADS) attn_long_bwd_dq_kernel(AttnLongArgs p) {
    p.drop = drop_resolve(p.drop);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int S = p.S, SP = (S + 31) & ~31, Sq = p.Sq;
    bf16_t* Ks = (bf16_t*)smem;
    bf16_t* Vs = Ks + SP * AL_ROW;
    int* traj_s = (int*)(Vs + SP * AL_ROW);
    unsigned* kv_s = (unsigned*)(traj_s + SP);       // one byte per key, read four at a time
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int ql = lane & 15, g = lane >> 4;
    const int r = blockIdx.x / p.H, h = blockIdx.x % p.H;
    const size_t tok0 = (size_t)r * S, qtok0 = (size_t)r * Sq;
    const int ntile = (Sq + 15) >> 4;
    // Q / dO fragments, the D partial and the LSE of query tile qt (lane: query qt*16 + ql, head dims 8g .. 8g+7 and 32 + 8g ..)
    auto load_q = [&](int qt) {
        const int q = qt * 16 + ql;
        const bool qok = qt < ntile && q < Sq;
        const size_t row = qtok0 + (qok ? q : 0);
        const bf16_t* qp = p.Q + row * p.ldq + h * AL_HD + 8 * g;
        const bf16_t* gp = p.dO + row * p.lddo + h * AL_HD + 8 * g;
        const bf16_t* op = p.O + row * p.ldo + h * AL_HD + 8 * g;
        AlQFrag f;
        f.q0 = gld8(qp, qok); f.q1 = gld8(qp + 32, qok);
        f.g0 = gld8(gp, qok); f.g1 = gld8(gp + 32, qok);
        f.d = dot8(f.g0, gld8(op, qok)) + dot8(f.g1, gld8(op + 32, qok));
        f.lse = qok ? p.LSE[((size_t)r * p.H + h) * Sq + q] : INFINITY;      // +inf => P = 0 for padded queries
        return f;
    };
    AlQFrag nxt = load_q(wid);      // in flight across the staging barrier
    al_stage(Ks, p.K + tok0 * p.ld + h * AL_HD, p.ld, S, SP, tid);
    al_stage(Vs, p.V + tok0 * p.ld + h * AL_HD, p.ld, S, SP, tid);
    for (int i = tid; i < SP; i += AL_THREADS) {
        traj_s[i] = (p.traj && i < S) ? p.traj[tok0 + i] : -1;
        ((unsigned char*)kv_s)[i] = i < S ? (p.kvalid ? (p.kvalid[tok0 + i] ? 1 : 0) : 1) : 0;
    }
    __syncthreads();
    const bool causal = p.mask_mode == MASK_BLOCK_CAUSAL;
    const RowBase Krow = att_row_base(Ks, lane), Vrow = att_row_base(Vs, lane);
    const TrBase Ktr = att_tr_base(Ks, lane);
    const float sl2 = p.scale * LOG2E;
    for (int qt = wid; qt < ntile; qt += AL_NW) {
        const AlQFrag cur = nxt;
        if (qt + AL_NW < ntile) nxt = load_q(qt + AL_NW);
        const int q = qt * 16 + ql;
        const bool qok = q < Sq;
        float D_q = cur.d;
        D_q += __shfl_xor(D_q, 16, 64);
        D_q += __shfl_xor(D_q, 32, 64);
        const float lse_q = cur.lse, lse2_q = cur.lse * LOG2E;
        const int tq = MASKED ? traj_s[qok ? q : 0] : 0;
        const unsigned long long rb = p.drop.thr ? att_drop_row(p.S, p.H, r, h, qok ? q : 0) : 0ull;
        f32x4 dq[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) dq[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
        // key tile pairs: all of them, or (block-causal) those that hold a key <= the tile's last query
        const int nu = causal ? min(SP >> 5, (qt >> 1) + 1) : (SP >> 5);
        for (int u = 0; u < nu; ++u) {
            float dsv[8];
#pragma unroll
            for (int e2 = 0; e2 < 2; ++e2) {
                const int k0 = 32 * u + 16 * e2;
                f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
                s = mfma16(lds_row8i(Krow.lo, k0), cur.q0, s);
                s = mfma16(lds_row8i(Krow.hi, k0), cur.q1, s);
                dp = mfma16(lds_row8i(Vrow.lo, k0), cur.g0, dp);
                dp = mfma16(lds_row8i(Vrow.hi, k0), cur.g1, dp);
                // s[e], dp[e]: key k0 + 4g + e, query q.  dP = keep/(1-p) * (dO V^T): the forward's keep-mask, regenerated
                const unsigned dkeep = p.drop.thr ? drop_keep4(p.drop, rb + k0 + 4 * g) : 0xfu;
                if constexpr (MASKED) {
                    const int4 tk = *(const int4*)(traj_s + k0 + 4 * g);
                    const unsigned kv4 = kv_s[(k0 >> 2) + g];
                    const int tke[4] = {tk.x, tk.y, tk.z, tk.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int key = k0 + 4 * g + e;
                        const bool mk = !qok || !((kv4 >> (8 * e)) & 0xffu) || (causal && (key > q || tke[e] != tq));
                        const float pr = mk ? 0.f : __expf(s[e] * p.scale - lse_q);
                        dsv[e2 * 4 + e] = pr * (((dkeep >> e) & 1u ? dp[e] * p.drop.scale : 0.f) - D_q) * p.scale;
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        dsv[e2 * 4 + e] = __builtin_amdgcn_exp2f(s[e] * sl2 - lse2_q) * (((dkeep >> e) & 1u ? dp[e] * p.drop.scale : 0.f) - D_q) * p.scale;
                }
            }
            const bf16x8 da = pack8(dsv);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) dq[dt] = mfma16(lds_tr8i(Ktr.d[dt], 32 * u, 32 * u + 16), da, dq[dt]);      // dQ^T: rows = head dims, cols = queries
        }
        if (qok) {
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const u32x2 w = {pack_bf2(dq[dt][0], dq[dt][1]), pack_bf2(dq[dt][2], dq[dt][3])};
                *(u32x2*)(p.dQ + (qtok0 + q) * p.lddq + h * AL_HD + dt * 16 + 4 * g) = w;
            }
        }
    }
}

// ================================================================================================ dK / dV
struct AlKVFrag { bf16x8 k0, k1, v0, v1; };

template <bool MASKED>
__global__ void __launch_bounds__(AL_THREADS) attn_long_bwd_dkv_kernel(AttnLongArgs p) {
    p.drop = drop_resolve(p.drop);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int S = p.S, SP = (S + 31) & ~31, Sq = p.Sq;
    bf16_t* Qs = (bf16_t*)smem;
    bf16_t* Gs = Qs + SP * AL_ROW;      // dO
    int* traj_s = (int*)(Gs + SP * AL_ROW);
    unsigned char* kv_s = (unsigned char*)(traj_s + SP);
    float* lse_s = (float*)(kv_s + SP);          // SP is a multiple of 32: 16-byte aligned
    float* D_s = lse_s + SP;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int ql = lane & 15, g = lane >> 4;
    const int r = blockIdx.x / p.H, h = blockIdx.x % p.H;
    const size_t tok0 = (size_t)r * S, qtok0 = (size_t)r * Sq;
    const int ntile = (S + 15) >> 4;
    // K / V B-operand fragments of key tile kt (lane: key kt*16 + ql)
    auto load_kv = [&](int kt) {
        const int keyl = kt * 16 + ql;
        const bool kok = kt < ntile && keyl < S;
        const bf16_t* kp = p.K + (tok0 + (kok ? keyl : 0)) * p.ld + h * AL_HD + 8 * g;
        const bf16_t* vp = p.V + (tok0 + (kok ? keyl : 0)) * p.ld + h * AL_HD + 8 * g;
        AlKVFrag f;
        f.k0 = gld8(kp, kok); f.k1 = gld8(kp + 32, kok);
        f.v0 = gld8(vp, kok); f.v1 = gld8(vp + 32, kok);
        return f;
    };
    AlKVFrag nxt = load_kv(wid);      // in flight across the staging barrier
    al_stage(Qs, p.Q + qtok0 * p.ldq + h * AL_HD, p.ldq, Sq, SP, tid);
    al_stage(Gs, p.dO + qtok0 * p.lddo + h * AL_HD, p.lddo, Sq, SP, tid);
    for (int i = tid; i < SP; i += AL_THREADS) {
        traj_s[i] = (p.traj && i < S) ? p.traj[tok0 + i] : -1;
        kv_s[i] = i < S ? (p.kvalid ? (p.kvalid[tok0 + i] ? 1 : 0) : 1) : 0;
        lse_s[i] = i < Sq ? p.LSE[((size_t)r * p.H + h) * Sq + i] * (MASKED ? 1.f : LOG2E) : INFINITY;      // +inf => P = 0 for padded queries
    }
    // D[q] = sum_d dO[q,d] * O[q,d]: 4 lanes per row (16 columns each); SP * 4 is a multiple of 128, so a wave is wholly inside or outside the loop
    for (int i = tid; i < SP * 4; i += AL_THREADS) {
        const int row = i >> 2, c = (i & 3) * 16;
        float v = 0.f;
        if (row < Sq) {
            const bf16_t* gp = p.dO + (qtok0 + row) * p.lddo + h * AL_HD + c;
            const bf16_t* op = p.O + (qtok0 + row) * p.ldo + h * AL_HD + c;
            v = dot8(*(const bf16x8*)gp, *(const bf16x8*)op) + dot8(*(const bf16x8*)(gp + 8), *(const bf16x8*)(op + 8));
        }
        v += __shfl_xor(v, 1, 64);
        v += __shfl_xor(v, 2, 64);
        if ((i & 3) == 0) D_s[row] = v;
    }
    __syncthreads();
    const bool causal = p.mask_mode == MASK_BLOCK_CAUSAL;
    const RowBase Qrow = att_row_base(Qs, lane), Grow = att_row_base(Gs, lane);
    const TrBase Qtr = att_tr_base(Qs, lane), Gtr = att_tr_base(Gs, lane);
    const float sl2 = p.scale * LOG2E;
    const unsigned SP4 = (unsigned)((S + 3) & ~3);
    const int nw = (Sq + 31) >> 5;      // query tile pairs that hold a query (<= SP / 32)
    for (int kt = wid; kt < ntile; kt += AL_NW) {
        const AlKVFrag cur = nxt;
        if (kt + AL_NW < ntile) nxt = load_kv(kt + AL_NW);
        const int keyl = kt * 16 + ql;      // this lane's key as the B-operand column
        const bool kok = keyl < S;
        const int tk = traj_s[keyl];
        const bool kvis = kok && kv_s[keyl];
        const unsigned long long eb = p.drop.thr ? att_drop_row(p.S, p.H, r, h, 0) + keyl : 0ull;      // element index of (query 0, this key); query q: + q * SP4 < 2^18
        f32x4 dk[4], dv[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) { dk[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; }
        // query tile pairs: all of them, or (block-causal) those that hold a query >= the tile's first key
        for (int w = causal ? (kt >> 1) : 0; w < nw; ++w) {
            float pv[8], dsv[8];
#pragma unroll
            for (int e2 = 0; e2 < 2; ++e2) {
                const int q0 = 32 * w + 16 * e2;
                f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
                s = mfma16(lds_row8i(Qrow.lo, q0), cur.k0, s);
                s = mfma16(lds_row8i(Qrow.hi, q0), cur.k1, s);
                dp = mfma16(lds_row8i(Grow.lo, q0), cur.v0, dp);
                dp = mfma16(lds_row8i(Grow.hi, q0), cur.v1, dp);
                // s[e], dp[e]: query q0 + 4g + e, key keyl
                const f32x4 l4 = *(const f32x4*)(lse_s + q0 + 4 * g), d4 = *(const f32x4*)(D_s + q0 + 4 * g);
                int tqe[4] = {0, 0, 0, 0};
                if constexpr (MASKED) {
                    const int4 tq = *(const int4*)(traj_s + q0 + 4 * g);
                    tqe[0] = tq.x; tqe[1] = tq.y; tqe[2] = tq.z; tqe[3] = tq.w;
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int q = q0 + 4 * g + e;
                    float pr;
                    if constexpr (MASKED) {
                        const bool mk = q >= Sq || !kvis || (causal && (keyl > q || tqe[e] != tk));
                        pr = mk ? 0.f : __expf(s[e] * p.scale - l4[e]);
                    } else {
                        pr = __builtin_amdgcn_exp2f(s[e] * sl2 - l4[e]);      // lse_s holds lse*log2e (+inf for padded queries); padded key columns are never stored
                    }
                    const bool kp = !p.drop.thr || att_keep1(p.drop, eb + (unsigned)(q < Sq ? q : 0) * SP4);
                    pv[e2 * 4 + e] = kp ? pr * p.drop.scale : 0.f;
                    dsv[e2 * 4 + e] = pr * ((kp ? dp[e] * p.drop.scale : 0.f) - d4[e]) * p.scale;
                }
            }
            const bf16x8 pa = pack8(pv), da = pack8(dsv);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                dv[dt] = mfma16(lds_tr8i(Gtr.d[dt], 32 * w, 32 * w + 16), pa, dv[dt]);      // dV^T / dK^T: rows = head dims, cols = keys
                dk[dt] = mfma16(lds_tr8i(Qtr.d[dt], 32 * w, 32 * w + 16), da, dk[dt]);
            }
        }
        if (kok) {
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const u32x2 wk = {pack_bf2(dk[dt][0], dk[dt][1]), pack_bf2(dk[dt][2], dk[dt][3])};
                const u32x2 wv = {pack_bf2(dv[dt][0], dv[dt][1]), pack_bf2(dv[dt][2], dv[dt][3])};
                *(u32x2*)(p.dK + (tok0 + keyl) * p.ldd + h * AL_HD + dt * 16 + 4 * g) = wk;
                *(u32x2*)(p.dV + (tok0 + keyl) * p.ldd + h * AL_HD + dt * 16 + 4 * g) = wv;
            }
        }
    }
}

// ================================================================================================ launcher
int attn_long_bwd_launch(const AttnCall& c) {
    if (!attn_accepts(c, ATTN_BWD_64_LONG)) return SVLA_EINVAL;
    const AttnLongArgs p = attn_fill<AttnLongArgs>(c);
    const int SP = (c.S + 31) & ~31;      // the LDS image grows with S: the opt-in follows the largest window seen
    const dim3 grid(c.rows * c.H), block(AL_THREADS);
    const bool generic = c.mask_mode != MASK_NONE || c.kvalid;
    if (const int rc = generic ? svla_launch<attn_long_bwd_dq_kernel<true>>(grid, block, al_lds_dq(SP), c.stream, p)
                               : svla_launch<attn_long_bwd_dq_kernel<false>>(grid, block, al_lds_dq(SP), c.stream, p)) return rc;
    return generic ? svla_launch<attn_long_bwd_dkv_kernel<true>>(grid, block, al_lds_dkv(SP), c.stream, p)
                   : svla_launch<attn_long_bwd_dkv_kernel<false>>(grid, block, al_lds_dkv(SP), c.stream, p);
}
