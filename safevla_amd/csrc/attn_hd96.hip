// Fused softmax attention for head_dim 96, forward + backward, bf16 in/out, fp32 scores / softmax / accumulators
// (gfx950, v_mfma_f32_16x16x32_bf16).  The imitation-learning presets base_6 and siglip_base_3_6 are TransformerConfig(n, 768, 8):
// eight heads of 96 in the fusion transformer (S = 1+84+84+L <= 256, no mask, dropout, pruned last layer Sq = 1) and, for base_6, in
// the llama decoder (S = T <= 256, block-causal on the trajectory ids, key padding).
//
// Same arithmetic contract as the 64-wide kernels of attn.hip (whose header describes the swapped QK^T layout): one workgroup owns one
// (batch row, head) with K and V resident in LDS, the whole score row of a 16-query tile lives in registers (exact two-pass softmax),
// the natural-log LSE is saved for the backward, probabilities are rounded to bf16 before P.V, the dropout element index is
// ((r*H + h)*S + q) * SP4 + k (include/svla.h: svla_dropout).  With 96 = 3 x 32 = 6 x 16 the QK^T reduction is three MFMA k-steps and
// P.V / dQ / dK / dV have six 16-column output tiles.  Not built at this width: the T5 bias, S > 256, the persistent / single-pass /
// decode variants and tower-grouped twins (plain launches, like the 64-wide backward).
//
// LDS image of one [SP, 96] head slice.  A row is 192 B = twelve 16-byte chunks, so the 8-chunk XOR of attn.hip does not carry over.
// The slice is stored as TWO PANELS, each with a power-of-two row and its own swizzle:
//   panel A: columns  0..63, [SP][64], 128-byte rows, chunk c -> c ^ fA(row), fA = att_swz of attn_common.h (x = (row >> 1) & 7 -> 0,2,4,6,5,7,1,3)
//   panel B: columns 64..95, [SP][32],  64-byte rows, chunk c -> c ^ fB(row), fB(y = (row >> 2) & 3) = 0,2,3,1
// 192 B per row, no padding: K + V are 72 KiB for S <= 192 (two workgroups per CU in 160 KiB) and 96 KiB for S <= 256 (one).
// Banks are (byte address / 4) mod 64 for every read used here, i.e. a 256-byte bank row holds two rows of panel A or four of panel B.
// What each access pattern asks of panel B (panel A: the derivation at att_swz in attn_common.h):
//  * ds_read_b128 row fragments of the third k-step (row = lane & 15, chunk = lane >> 4): the hardware serves the 16-lane groups
//    {0-3,12-15,20-27}, {4-11,16-19,28-31}, ...: rows {0-3,12-15} on chunk c together with rows {4-11} on chunk c ^ 1.  Rows j, j+4,
//    j+8, j+12 share the 64-byte bank quarter j & 3, so their four 16-byte slots must differ:
//    fB(0), fB(3), 1 ^ fB(1), 1 ^ fB(2) pairwise distinct;
//  * ds_read_b64_tr_b16 (32 lanes per pass = 8 rows x 32 B = one chunk PAIR per row): rows j and j+4 share a bank quarter, so
//    fB >> 1 must differ between y = 0 and 1 and between y = 2 and 3;
//  * staging stores (ds_write_b128, 8 lanes = two whole rows = 128 contiguous bytes): any fB.
// fB = 0,2,3,1 satisfies all three (1 ^ fB(1) = 3, 1 ^ fB(2) = 2); both panels are conflict-free for both kinds of read under the
// bank rule above.
#include "attn_host.h"      // AttnCall; attn_common.h: dropout index, panel A's swizzle (att_swz), fragment helpers

#define HD96 96
#define A96_THREADS 256

struct Attn96Args {
    const bf16_t *Q, *K, *V; long ld;     // token row stride (elements) of the k/v tensors
    bf16_t* O; long ldo;
    float* LSE;                           // [rows, H, Sq]
    const bf16_t* dO; long lddo;
    bf16_t *dQ, *dK, *dV; long ldd;
    const int* traj;                      // [rows, S] (block-causal)
    const unsigned char* kvalid;          // [rows, S] key padding mask or null
    int S, H, mask_mode;
    float scale;
    int kv_rows;                          // K/V token rows allocated per batch row (>= S)
    int Sq;                               // query rows per batch row present in Q / O / dO / dQ / LSE
    long ldq, lddq;
    float* Dws;                           // [rows, H, Sq] rowsum(dO * O): written by the dQ kernel, read by the dK/dV kernel (or null)
    DropCfg drop;
};

__device__ __forceinline__ int a96_swz_b(int row) { return (0x78 >> (((row >> 2) & 3) << 1)) & 3; }      // 0,2,3,1

// One head slice in LDS: panel A at the base, panel B behind it.  Tile rows are multiples of 16 and both swizzles have period 16, so the
// swizzle term of a lane base depends on the lane only and the tile offset stays a compile-time immediate of the ds_read.
template <int SP> struct A96Img {
    static constexpr int ELEMS = SP * HD96;
    static constexpr int PANEL_B = SP * 64;
};
//   row fragment : row = tile + (lane & 15), k-step ks = logical chunk (lane >> 4) + 4 ks
//   transposed   : row = tile + 4 (lane >> 4) + ((lane & 15) >> 2), columns dt*16 + 4 ((lane & 15) & 3) .. +3
struct Row96 { const bf16_t* k[3]; };
template <int SP>
__device__ __forceinline__ Row96 a96_row_base(const bf16_t* img, int lane) {
    const int ql = lane & 15, g = lane >> 4, fa = att_swz(ql), fb = a96_swz_b(ql);
    return Row96{{img + ql * 64 + ((g ^ fa) << 3), img + ql * 64 + (((g + 4) ^ fa) << 3), img + A96Img<SP>::PANEL_B + ql * 32 + ((g ^ fb) << 3)}};
}
struct Tr96 { const bf16_t* d[6]; };
template <int SP>
__device__ __forceinline__ Tr96 a96_tr_base(const bf16_t* img, int lane) {
    const int ql = lane & 15, g = lane >> 4;
    const int row = 4 * g + (ql >> 2), fa = att_swz(row), fb = a96_swz_b(row);
    const int hi = (ql & 3) >> 1, sub = 4 * (ql & 1);
    Tr96 t;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) t.d[dt] = img + row * 64 + (((2 * dt + hi) ^ fa) << 3) + sub;
#pragma unroll
    for (int dt = 4; dt < 6; ++dt) t.d[dt] = img + A96Img<SP>::PANEL_B + row * 32 + (((2 * (dt - 4) + hi) ^ fb) << 3) + sub;
    return t;
}
// A-operand row fragment of k-step KS (compile-time) for the tile that starts at row tile_row0
template <int KS>
__device__ __forceinline__ bf16x8 a96_row8(const Row96& b, int tile_row0) {
    return *(const bf16x8*)(b.k[KS] + tile_row0 * (KS < 2 ? 64 : 32));
}
// B/A-operand gather of output tile DT: 8 reduction slots = rows {rA + 4g + 0..3, rB + 4g + 0..3}, column DT*16 + (lane & 15)
template <int DT>
__device__ __forceinline__ bf16x8 a96_tr8(const Tr96& b, int rA, int rB) {
    constexpr int stride = DT < 4 ? 64 : 32;
    const bf16x4 lo = lds_tr16_b64(b.d[DT] + rA * stride);
    const bf16x4 hi = lds_tr16_b64(b.d[DT] + rB * stride);
    return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
// acc[dt] += X^T tile dt . frag for the six output tiles (X = the LDS image behind b, reduction rows 32 u .. 32 u + 31)
__device__ __forceinline__ void a96_mma6(f32x4 (&acc)[6], const Tr96& b, int u, bf16x8 frag) {
    acc[0] = mfma16(a96_tr8<0>(b, 32 * u, 32 * u + 16), frag, acc[0]);
    acc[1] = mfma16(a96_tr8<1>(b, 32 * u, 32 * u + 16), frag, acc[1]);
    acc[2] = mfma16(a96_tr8<2>(b, 32 * u, 32 * u + 16), frag, acc[2]);
    acc[3] = mfma16(a96_tr8<3>(b, 32 * u, 32 * u + 16), frag, acc[3]);
    acc[4] = mfma16(a96_tr8<4>(b, 32 * u, 32 * u + 16), frag, acc[4]);
    acc[5] = mfma16(a96_tr8<5>(b, 32 * u, 32 * u + 16), frag, acc[5]);
}
// acc += X[tile rows, :] . frag^T over the three k-steps
__device__ __forceinline__ f32x4 a96_dot3(const Row96& b, int tile_row0, const bf16x8 (&frag)[3], f32x4 acc) {
    acc = mfma16(a96_row8<0>(b, tile_row0), frag[0], acc);
    acc = mfma16(a96_row8<1>(b, tile_row0), frag[1], acc);
    acc = mfma16(a96_row8<2>(b, tile_row0), frag[2], acc);
    return acc;
}
// this lane's three k-step fragments of one 96-wide token row (columns 8g, 32 + 8g, 64 + 8g): zero when !ok
__device__ __forceinline__ void a96_gld_row(bf16x8 (&dst)[3], const bf16_t* row_g, bool ok) {
    dst[0] = gld8(row_g, ok); dst[1] = gld8(row_g + 32, ok); dst[2] = gld8(row_g + 64, ok);
}
// 8-byte stores of the six output tiles: acc[dt][e] = column dt*16 + 4g + e of this lane's token row
__device__ __forceinline__ void a96_store_row(bf16_t* row_g4, const f32x4 (&acc)[6], float mul) {
#pragma unroll
    for (int dt = 0; dt < 6; ++dt) {
        const u32x2 w = {pack_bf2(acc[dt][0] * mul, acc[dt][1] * mul), pack_bf2(acc[dt][2] * mul, acc[dt][3] * mul)};
        *(u32x2*)(row_g4 + dt * 16) = w;
    }
}

// stage an [n, 96] head slice into its LDS image (zero-filled up to SP rows; SP is a multiple of 64): 16-byte global loads, all of them
// issued before the first LDS store so the HBM / L2 latency is paid once
template <int SP>
__device__ __forceinline__ void a96_stage(bf16_t* img, const bf16_t* src, long ld, int n, int tid) {
    constexpr int ITA = SP * 8 / A96_THREADS, ITB = SP * 4 / A96_THREADS;
    u32x4 wa[ITA], wb[ITB];
#pragma unroll
    for (int i = 0; i < ITA; ++i) {
        const int q = tid + i * A96_THREADS, row = q >> 3, c = q & 7;
        wa[i] = u32x4{0, 0, 0, 0};
        if (row < n) wa[i] = *(const u32x4*)(src + (size_t)row * ld + c * 8);
    }
#pragma unroll
    for (int i = 0; i < ITB; ++i) {
        const int q = tid + i * A96_THREADS, row = q >> 2, c = q & 3;
        wb[i] = u32x4{0, 0, 0, 0};
        if (row < n) wb[i] = *(const u32x4*)(src + (size_t)row * ld + 64 + c * 8);
    }
#pragma unroll
    for (int i = 0; i < ITA; ++i) {
        const int q = tid + i * A96_THREADS, row = q >> 3;
        *(u32x4*)(img + row * 64 + (((q & 7) ^ att_swz(row)) << 3)) = wa[i];
    }
#pragma unroll
    for (int i = 0; i < ITB; ++i) {
        const int q = tid + i * A96_THREADS, row = q >> 2;
        *(u32x4*)(img + A96Img<SP>::PANEL_B + row * 32 + (((q & 3) ^ a96_swz_b(row)) << 3)) = wb[i];
    }
}

// ================================================================================================ forward
// GENERIC = false: no trajectory / padding mask (the fusion layers): only the ragged tail of the key range is masked and the softmax
// runs in the exp2 domain with the scale folded in.  Waves own query tiles qt = wid, wid + 4, ...
template <int NKT, bool GENERIC>
__global__ void __launch_bounds__(A96_THREADS, NKT <= 12 ? 2 : 1) attn96_fwd_kernel(Attn96Args p) {
    p.drop = drop_resolve(p.drop);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int SP = NKT * 16;
    bf16_t* Ks = (bf16_t*)smem;
    bf16_t* Vs = Ks + A96Img<SP>::ELEMS;
    int* traj_s = (int*)(Vs + A96Img<SP>::ELEMS);
    unsigned char* kv_s = (unsigned char*)(traj_s + SP);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int r = blockIdx.x / p.H, h = blockIdx.x % p.H;
    const size_t tok0 = (size_t)r * p.kv_rows, mtok0 = (size_t)r * p.S;
    const int S = p.S;
    a96_stage<SP>(Ks, p.K + tok0 * p.ld + h * HD96, p.ld, S, tid);
    a96_stage<SP>(Vs, p.V + tok0 * p.ld + h * HD96, p.ld, S, tid);
    if constexpr (GENERIC) {
        for (int i = tid; i < SP; i += A96_THREADS) {
            traj_s[i] = (p.traj && i < S) ? p.traj[mtok0 + i] : -1;
            kv_s[i] = (p.kvalid && i < S) ? p.kvalid[mtok0 + i] : 1;
        }
    }
    const int ql = lane & 15, g = lane >> 4;
    const int Sq = p.Sq;
    const size_t qtok0 = (size_t)r * Sq;
    const int nqt = (Sq + 15) / 16;
    // Q fragments of this wave's query tiles (qt = wid, wid + 4, ...): the first tile's are issued before the barrier so their latency
    // overlaps the K/V staging, tile t+1's at the top of tile t (two register sets, not MAXQT: the S <= 256 masked form must not spill)
    constexpr int MAXQT = (NKT + 3) / 4;
    bf16x8 qbuf[2][3];
    auto load_q = [&](int t, bf16x8 (&dst)[3]) {
        const int q = (wid + 4 * t) * 16 + ql;
        const bool ok = q < Sq;
        a96_gld_row(dst, p.Q + (qtok0 + (ok ? q : 0)) * p.ldq + h * HD96 + 8 * g, ok);
    };
    load_q(0, qbuf[0]);
    __syncthreads();
    const unsigned char* kvp = p.kvalid ? kv_s : nullptr;
    const Row96 Krow = a96_row_base<SP>(Ks, lane);
    const Tr96 Vtr = a96_tr_base<SP>(Vs, lane);
    const float sl2 = p.scale * LOG2E;      // scores are kept in the log2 domain: p = exp2(s*scale*log2e - max)
#pragma unroll
    for (int t = 0; t < MAXQT; ++t) {
        const int qt = wid + 4 * t;
        if (qt >= nqt) break;
        const int q = qt * 16 + ql;
        if (t + 1 < MAXQT && qt + 4 < nqt) load_q(t + 1, qbuf[(t + 1) & 1]);
        const bf16x8 (&qf)[3] = qbuf[t & 1];
        float sc[NKT][4];
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
            f32x4 a = {0.f, 0.f, 0.f, 0.f};
            if (kt * 16 < S) a = a96_dot3(Krow, kt * 16, qf, a);
            if constexpr (GENERIC) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float s = a[e] * sl2;
                    if (att_masked(p, q < Sq ? q : 0, kt * 16 + 4 * g + e, traj_s, kvp)) s = -INFINITY;
                    sc[kt][e] = s;
                    mx = fmaxf(mx, s);
                }
            } else {
                const bool tail = (kt + 1) * 16 > S;      // wave-uniform: only the last (ragged) key tiles need masking
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float s = a[e] * sl2;
                    if (tail && kt * 16 + 4 * g + e >= S) s = -INFINITY;
                    sc[kt][e] = s;
                    mx = fmaxf(mx, s);
                }
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        if (mx == -INFINITY) mx = 0.f;
        float lsum = 0.f;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int e = 0; e < 4; ++e) { sc[kt][e] = __builtin_amdgcn_exp2f(sc[kt][e] - mx); lsum += sc[kt][e]; }
        lsum += __shfl_xor(lsum, 16, 64);
        lsum += __shfl_xor(lsum, 32, 64);
        if (p.drop.thr) {      // dropout on the normalised probabilities: zero here, 1/(1-p) folded into the final scale
            const unsigned long long rb = att_drop_row(p.S, p.H, r, h, q < Sq ? q : 0);
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt) {
                const unsigned keep = drop_keep4(p.drop, rb + kt * 16 + 4 * g);
#pragma unroll
                for (int e = 0; e < 4; ++e) if (!((keep >> e) & 1u)) sc[kt][e] = 0.f;
            }
        }
        f32x4 o[6];
#pragma unroll
        for (int dt = 0; dt < 6; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < NKT / 2; ++u) {
            if (u * 32 < S) {
                const float pv[8] = {sc[2 * u][0], sc[2 * u][1], sc[2 * u][2], sc[2 * u][3],
                                     sc[2 * u + 1][0], sc[2 * u + 1][1], sc[2 * u + 1][2], sc[2 * u + 1][3]};
                a96_mma6(o, Vtr, u, pack8(pv));      // O^T: rows = head dims, cols = queries
            }
        }
        const float inv = lsum > 0.f ? p.drop.scale / lsum : 0.f;
        if (q < Sq) a96_store_row(p.O + (qtok0 + q) * p.ldo + h * HD96 + 4 * g, o, inv);
        if (p.LSE && g == 0 && q < Sq) p.LSE[((size_t)r * p.H + h) * Sq + q] = (mx + __log2f(lsum)) * LN2;   // natural-log LSE
    }
}

// ================================================================================================ backward
// Two kernels, each with two [S, 96] operands resident in LDS:
//   dQ  kernel (waves own query tiles, swapped layout, K and V in LDS):   dQ = dS.K
//   dKV kernel (waves own key tiles, Q and dO in LDS):                    dK = dS^T.Q, dV = P^T.dO
// P is recomputed from the saved log-sum-exp; D = rowsum(dO * O) is handed from the first to the second through Dws when given.
template <int NKT, bool GENERIC>
__global__ void __launch_bounds__(A96_THREADS, NKT <= 12 ? 2 : 1) attn96_bwd_dq_kernel(Attn96Args p) {
    p.drop = drop_resolve(p.drop);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int SP = NKT * 16;
    bf16_t* Ks = (bf16_t*)smem;
    bf16_t* Vs = Ks + A96Img<SP>::ELEMS;
    int* traj_s = (int*)(Vs + A96Img<SP>::ELEMS);
    unsigned char* kv_s = (unsigned char*)(traj_s + SP);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int r = blockIdx.x / p.H, h = blockIdx.x % p.H;
    const size_t tok0 = (size_t)r * p.S;
    const int S = p.S;
    a96_stage<SP>(Ks, p.K + tok0 * p.ld + h * HD96, p.ld, S, tid);
    a96_stage<SP>(Vs, p.V + tok0 * p.ld + h * HD96, p.ld, S, tid);
    if constexpr (GENERIC) {
        for (int i = tid; i < SP; i += A96_THREADS) {
            traj_s[i] = (p.traj && i < S) ? p.traj[tok0 + i] : -1;
            kv_s[i] = (p.kvalid && i < S) ? p.kvalid[tok0 + i] : 1;
        }
    }
    const int ql = lane & 15, g = lane >> 4;
    const int Sq = p.Sq;
    const size_t qtok0 = (size_t)r * Sq;
    const unsigned char* kvp = p.kvalid ? kv_s : nullptr;
    const Row96 Krow = a96_row_base<SP>(Ks, lane), Vrow = a96_row_base<SP>(Vs, lane);
    const Tr96 Ktr = a96_tr_base<SP>(Ks, lane);
    const int ntile = (Sq + 15) / 16;
    const float sl2 = p.scale * LOG2E;
    constexpr int MAXQT = (NKT + 3) / 4;
    // Q / dO fragments, D partial and LSE of one query tile; the first tile's are issued ahead of the staging barrier, tile t+1's at the
    // top of tile t
    bf16x8 qbuf[2][3], gbuf[2][3];
    float dbuf[2], lbuf[2];
    auto load_q = [&](int t, bf16x8 (&qd)[3], bf16x8 (&gd)[3], float& dd, float& ll) {
        const int q = (wid + 4 * t) * 16 + ql;
        const bool qok = q < Sq;
        const size_t tok = qtok0 + (qok ? q : 0);
        bf16x8 of[3];
        a96_gld_row(qd, p.Q + tok * p.ldq + h * HD96 + 8 * g, qok);
        a96_gld_row(gd, p.dO + tok * p.lddo + h * HD96 + 8 * g, qok);
        a96_gld_row(of, p.O + tok * p.ldo + h * HD96 + 8 * g, qok);
        dd = dot8(gd[0], of[0]) + dot8(gd[1], of[1]) + dot8(gd[2], of[2]);
        ll = qok ? p.LSE[((size_t)r * p.H + h) * Sq + q] : INFINITY;
    };
    load_q(0, qbuf[0], gbuf[0], dbuf[0], lbuf[0]);
    __syncthreads();
#pragma unroll
    for (int t = 0; t < MAXQT; ++t) {
        const int qt = wid + 4 * t;
        if (qt >= ntile) break;
        const int q = qt * 16 + ql;
        const bool qok = q < Sq;
        if (t + 1 < MAXQT && qt + 4 < ntile) load_q(t + 1, qbuf[(t + 1) & 1], gbuf[(t + 1) & 1], dbuf[(t + 1) & 1], lbuf[(t + 1) & 1]);
        const bf16x8 (&qf)[3] = qbuf[t & 1];
        const bf16x8 (&gf)[3] = gbuf[t & 1];
        float D_q = dbuf[t & 1];
        D_q += __shfl_xor(D_q, 16, 64);
        D_q += __shfl_xor(D_q, 32, 64);
        if (p.Dws && g == 0 && qok) p.Dws[((size_t)r * p.H + h) * Sq + q] = D_q;
        const float lse_q = lbuf[t & 1], lse2_q = lse_q * LOG2E;
        f32x4 dq[6];
#pragma unroll
        for (int dt = 0; dt < 6; ++dt) dq[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < NKT / 2; ++u) {
            if (u * 32 < S) {
                float dsv[8];
#pragma unroll
                for (int e2 = 0; e2 < 2; ++e2) {
                    const int kt = 2 * u + e2;
                    const f32x4 s = a96_dot3(Krow, kt * 16, qf, f32x4{0.f, 0.f, 0.f, 0.f});
                    const f32x4 dp = a96_dot3(Vrow, kt * 16, gf, f32x4{0.f, 0.f, 0.f, 0.f});
                    // dP = keep/(1-p) * (dO V^T): the forward's keep-mask, regenerated
                    const unsigned dkeep = p.drop.thr ? drop_keep4(p.drop, att_drop_row(p.S, p.H, r, h, qok ? q : 0) + kt * 16 + 4 * g) : 0xfu;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float pr;
                        if constexpr (GENERIC) {
                            const bool mk = !qok || att_masked(p, qok ? q : 0, kt * 16 + 4 * g + e, traj_s, kvp);
                            pr = mk ? 0.f : __builtin_amdgcn_exp2f(s[e] * sl2 - lse2_q);
                        } else {
                            // no mask needed: padded keys have zero K rows (their dS never reaches dQ), padded queries have lse = +inf => P = 0
                            pr = __builtin_amdgcn_exp2f(s[e] * sl2 - lse2_q);
                        }
                        dsv[e2 * 4 + e] = pr * (((dkeep >> e) & 1u ? dp[e] * p.drop.scale : 0.f) - D_q) * p.scale;
                    }
                }
                a96_mma6(dq, Ktr, u, pack8(dsv));      // dQ^T: rows = head dims, cols = queries
            }
        }
        if (qok) a96_store_row(p.dQ + (qtok0 + q) * p.lddq + h * HD96 + 4 * g, dq, 1.f);
    }
}

template <int NKT, bool GENERIC>
__global__ void __launch_bounds__(A96_THREADS, NKT <= 12 ? 2 : 1) attn96_bwd_dkv_kernel(Attn96Args p) {
    p.drop = drop_resolve(p.drop);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int SP = NKT * 16;
    bf16_t* Qs = (bf16_t*)smem;
    bf16_t* Gs = Qs + A96Img<SP>::ELEMS;  // dO
    float* lse_s = (float*)(Gs + A96Img<SP>::ELEMS);
    float* D_s = lse_s + SP;
    int* traj_s = (int*)(D_s + SP);
    unsigned char* kv_s = (unsigned char*)(traj_s + SP);
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int r = blockIdx.x / p.H, h = blockIdx.x % p.H;
    const size_t tok0 = (size_t)r * p.S;
    const int S = p.S;
    // this wave's K/V B-operand fragments: the first key tile's are issued ahead of the staging barrier, tile t+1's at the top of tile t
    constexpr int MAXKT = (NKT + 3) / 4;
    bf16x8 kbuf[2][3], vbuf[2][3];
    auto load_kv = [&](int t, bf16x8 (&kd)[3], bf16x8 (&vd)[3]) {
        const int keyl = (wid + 4 * t) * 16 + (lane & 15);
        const bool kok = keyl < S;
        const size_t off = (tok0 + (kok ? keyl : 0)) * p.ld + h * HD96 + 8 * (lane >> 4);
        a96_gld_row(kd, p.K + off, kok);
        a96_gld_row(vd, p.V + off, kok);
    };
    load_kv(0, kbuf[0], vbuf[0]);
    const int Sq = p.Sq;
    const size_t qtok0 = (size_t)r * Sq;
    a96_stage<SP>(Qs, p.Q + qtok0 * p.ldq + h * HD96, p.ldq, Sq, tid);
    a96_stage<SP>(Gs, p.dO + qtok0 * p.lddo + h * HD96, p.lddo, Sq, tid);
    for (int i = tid; i < SP; i += A96_THREADS) {
        if constexpr (GENERIC) {
            traj_s[i] = (p.traj && i < S) ? p.traj[tok0 + i] : -1;
            kv_s[i] = (p.kvalid && i < S) ? p.kvalid[tok0 + i] : 1;
        }
        lse_s[i] = i < Sq ? p.LSE[((size_t)r * p.H + h) * Sq + i] * LOG2E : INFINITY;      // +inf => P = 0 for padded queries
        if (p.Dws) D_s[i] = i < Sq ? p.Dws[((size_t)r * p.H + h) * Sq + i] : 0.f;
    }
    if (!p.Dws) {   // D[q] = sum_d dO[q,d] * O[q,d]: 4 lanes per row (24 columns each), all rows' loads in flight at once
        constexpr int IT = SP * 4 / A96_THREADS;
        float part[IT];
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            const int q = tid + i * A96_THREADS;
            const int row = q >> 2, c = (q & 3) * 24;
            part[i] = 0.f;
            if (row < Sq) {
                const bf16_t* gp = p.dO + (qtok0 + row) * p.lddo + h * HD96 + c;
                const bf16_t* op = p.O + (qtok0 + row) * p.ldo + h * HD96 + c;
                part[i] = dot8(*(const bf16x8*)gp, *(const bf16x8*)op) + dot8(*(const bf16x8*)(gp + 8), *(const bf16x8*)(op + 8)) +
                          dot8(*(const bf16x8*)(gp + 16), *(const bf16x8*)(op + 16));
            }
        }
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            float v = part[i];
            v += __shfl_xor(v, 1, 64);
            v += __shfl_xor(v, 2, 64);
            const int q = tid + i * A96_THREADS;
            if ((q & 3) == 0) D_s[q >> 2] = v;
        }
    }
    __syncthreads();
    const unsigned char* kvp = p.kvalid ? kv_s : nullptr;
    const int ql = lane & 15, g = lane >> 4;
    const int ntile = (S + 15) / 16;
    const float sl2 = p.scale * LOG2E;
    const Row96 Qrow = a96_row_base<SP>(Qs, lane), Grow = a96_row_base<SP>(Gs, lane);
    const Tr96 Qtr = a96_tr_base<SP>(Qs, lane), Gtr = a96_tr_base<SP>(Gs, lane);
#pragma unroll
    for (int t = 0; t < MAXKT; ++t) {
        const int kt = wid + 4 * t;
        if (kt >= ntile) break;
        const int keyl = kt * 16 + ql;  // this lane's key as the B-operand column
        const bool kok = keyl < S;
        if (t + 1 < MAXKT && kt + 4 < ntile) load_kv(t + 1, kbuf[(t + 1) & 1], vbuf[(t + 1) & 1]);
        const bf16x8 (&kf)[3] = kbuf[t & 1];
        const bf16x8 (&vf)[3] = vbuf[t & 1];
        f32x4 dk[6], dv[6];
#pragma unroll
        for (int dt = 0; dt < 6; ++dt) { dk[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[dt] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
        for (int w = 0; w < NKT / 2; ++w) {
            if (w * 32 < Sq) {
                float pv[8], dsv[8];
#pragma unroll
                for (int e2 = 0; e2 < 2; ++e2) {
                    const int qt = 2 * w + e2;
                    const f32x4 s = a96_dot3(Qrow, qt * 16, kf, f32x4{0.f, 0.f, 0.f, 0.f});
                    const f32x4 dp = a96_dot3(Grow, qt * 16, vf, f32x4{0.f, 0.f, 0.f, 0.f});
                    // s[e]: query qt*16 + 4g + e, key keyl; lse_s holds lse*log2e (+inf for padded queries => P = 0); padded key columns are never stored
                    const f32x4 l4 = *(const f32x4*)(lse_s + 4 * g + qt * 16), d4 = *(const f32x4*)(D_s + 4 * g + qt * 16);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int q = qt * 16 + 4 * g + e;
                        float pr = __builtin_amdgcn_exp2f(s[e] * sl2 - l4[e]);
                        if constexpr (GENERIC) {
                            if (q >= Sq || att_masked(p, q < Sq ? q : 0, keyl, traj_s, kvp)) pr = 0.f;
                        }
                        const bool kp = !p.drop.thr || att_keep1(p.drop, att_drop_row(p.S, p.H, r, h, q < Sq ? q : 0) + keyl);
                        pv[e2 * 4 + e] = kp ? pr * p.drop.scale : 0.f;
                        dsv[e2 * 4 + e] = pr * ((kp ? dp[e] * p.drop.scale : 0.f) - d4[e]) * p.scale;
                    }
                }
                a96_mma6(dv, Gtr, w, pack8(pv));       // dV^T / dK^T: rows = head dims, cols = keys
                a96_mma6(dk, Qtr, w, pack8(dsv));
            }
        }
        if (kok) {
            a96_store_row(p.dK + (tok0 + keyl) * p.ldd + h * HD96 + 4 * g, dk, 1.f);
            a96_store_row(p.dV + (tok0 + keyl) * p.ldd + h * HD96 + 4 * g, dv, 1.f);
        }
    }
}

// ================================================================================================ launchers
template <int NKT> constexpr size_t a96_lds_kv() { return (size_t)2 * NKT * 16 * HD96 * sizeof(bf16_t) + NKT * 16 * (sizeof(int) + 1); }
template <int NKT> constexpr size_t a96_lds_dkv() { return a96_lds_kv<NKT>() + NKT * 16 * 2 * sizeof(float); }

template <int NKT>
static int a96_launch_fwd(const Attn96Args& p, int rows, hipStream_t st) {
    constexpr size_t lds = a96_lds_kv<NKT>();
    const dim3 grid(rows * p.H > 0 ? rows * p.H : 1);      // one workgroup per (row, head); rows, H >= 1 is checked by the caller
    if (p.mask_mode != MASK_NONE || p.kvalid) return svla_launch<attn96_fwd_kernel<NKT, true>>(grid, dim3(A96_THREADS), lds, st, p);
    return svla_launch<attn96_fwd_kernel<NKT, false>>(grid, dim3(A96_THREADS), lds, st, p);
}
template <int NKT>
static int a96_launch_bwd(const Attn96Args& p, int rows, hipStream_t st) {
    constexpr size_t lds_q = a96_lds_kv<NKT>(), lds_kv = a96_lds_dkv<NKT>();
    const dim3 grid(rows * p.H > 0 ? rows * p.H : 1), block(A96_THREADS);
    const bool generic = p.mask_mode != MASK_NONE || p.kvalid;
    if (const int rc = generic ? svla_launch<attn96_bwd_dq_kernel<NKT, true>>(grid, block, lds_q, st, p)
                               : svla_launch<attn96_bwd_dq_kernel<NKT, false>>(grid, block, lds_q, st, p)) return rc;
    return generic ? svla_launch<attn96_bwd_dkv_kernel<NKT, true>>(grid, block, lds_kv, st, p)
                   : svla_launch<attn96_bwd_dkv_kernel<NKT, false>>(grid, block, lds_kv, st, p);
}

int attn96_fwd_launch(const AttnCall& c) {
    if (!attn_accepts(c, ATTN_FWD_96)) return SVLA_EINVAL;
    Attn96Args p = attn_fill<Attn96Args>(c);
    p.kv_rows = attn_kv_rows(c);
    return attn_bucket<4, 8, 12, 16>(c.S, [&](auto nkt) { return a96_launch_fwd<nkt()>(p, c.rows, c.stream); });
}

int attn96_bwd_launch(const AttnCall& c) {
    if (!attn_accepts(c, ATTN_BWD_96)) return SVLA_EINVAL;
    Attn96Args p = attn_fill<Attn96Args>(c);
    p.kv_rows = c.S; p.Dws = c.D_ws;
    return attn_bucket<4, 8, 12, 16>(c.S, [&](auto nkt) { return a96_launch_bwd<nkt()>(p, c.rows, c.stream); });
}
