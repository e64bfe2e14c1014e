// Last fusion layer, one query per row (allenact_dino_transformer.py:545-552, 708: only x[:, 0] of the fusion encoder's output is consumed), with the
// K and V projections absorbed into the query side: per (row r, head h)
//     qt_h = W_k,h^T q_h            s_hj = scale * qt_h . x_j   (+ a term without j, which the softmax drops)
//     c_h  = sum_j pd_hj x_j        sigma_h = sum_j pd_hj        pd = keep / (1 - p) * softmax(s)        o_h = W_v,h c_h + sigma_h b_v,h
// so K and V never exist.  The small per-head products (qt, o and their gradients) run on the GEMM entry points over head-expanded [8 rows, 512] operands
// (head_expand / head_pick below); the two streaming kernels here touch the [S, 512] tokens of a row.
//
// One workgroup of 8 waves per row, S <= 256, 8 heads of 64 (D = 512):
//   * the score-like product ([S, 512] . [512, 8]: s, and dpd = dc . x in the backward) is MFMA: A = 16 tokens x 32 features straight from global memory in
//     fragment order, B = the 8 head vectors in columns 0 .. 7 (columns 8 .. 15 repeat them and are dropped); wave w takes the token tiles w and w + 8
//   * every product that sums over tokens (c, dqt) or over heads (dX) is VALU on "feature slices": lane l holds features 8 l .. 8 l + 7 of the tokens
//     w, w + 8, ... of its wave IN REGISTERS (32 x 16 B) from the forward's c (the backward's dqt) on.  Each row is loaded twice, once in each order, the
//     slices right after the fragments; measured, L2 serves only part of the second load (profiles/attn_q1_ab.txt: 1.6 .. 1.7 x the bytes of one pass fetched)
//   * softmax / dropout / dS: wave h owns head h, lane l the keys l, l + 64, ...; the keep decision is att_keep1(att_drop_row(S, 8, r, h, 0) + j) -- the
//     single-query case of attn.hip, bit for bit
//   * per-wave partial sums of c / dqt meet in an LDS tree (8 -> 4 -> 2 -> 1 waves); every output element has one writer, no atomics.
#include "attn_common.h"

#define Q1_D 512
#define Q1_H 8
#define Q1_WAVES 8
#define Q1_THREADS (Q1_WAVES * 64)
#define Q1_SMAX 256
#define Q1_SLOTS (Q1_SMAX / Q1_WAVES)                 // tokens a wave holds
#define Q1_RED_FLOATS (Q1_H * Q1_D)                   // one wave's [8, 512] partial
#define Q1_LDS_FWD ((size_t)(Q1_SMAX * Q1_H + 4 * Q1_RED_FLOATS) * sizeof(float))
#define Q1_LDS_BWD ((size_t)(2 * Q1_SMAX * Q1_H + 4 * Q1_RED_FLOATS) * sizeof(float))

__device__ __forceinline__ void q1_unpack(bf16x8 v, float (&f)[8]) {
    const u32x4 w = __builtin_bit_cast(u32x4, v);
#pragma unroll
    for (int i = 0; i < 4; ++i) { f[2 * i] = bf_lo(w[i]); f[2 * i + 1] = bf_hi(w[i]); }
}

// out[j][h] (LDS, [Q1_SMAX][8] floats) = mul * sum_d X[j, d] * V[h, d] for the token tiles of wave w; X: the row's tokens, V: [8, 512].  No load is predicated
// (a predicated load makes the compiler wait for each one): tile rows past the row -- a whole tile of them for the waves without a second tile -- re-read token
// S - 1 and columns 8 .. 15 re-read heads 0 .. 7; the results of both are dropped.
__device__ __forceinline__ void q1_token_head_products(const bf16_t* __restrict__ X, const bf16_t* __restrict__ V, int S, float mul, float* out, int w, int lane) {
    constexpr int NT = Q1_SMAX / (16 * Q1_WAVES), NK = Q1_D / 32;
    const int ql = lane & 15, g = lane >> 4;
    const bf16_t* vb = V + (size_t)(ql & (Q1_H - 1)) * Q1_D + 8 * g;
    bf16x8 a[NT][NK], b[NK];                              // every fragment of both tiles in flight at once: one memory round trip
#pragma unroll
    for (int tt = 0; tt < NT; ++tt) {
        const bf16_t* xa = X + (size_t)min((w + Q1_WAVES * tt) * 16 + ql, S - 1) * Q1_D + 8 * g;
#pragma unroll
        for (int kk = 0; kk < NK; ++kk) a[tt][kk] = *(const bf16x8*)(xa + kk * 32);
    }
#pragma unroll
    for (int kk = 0; kk < NK; ++kk) b[kk] = *(const bf16x8*)(vb + kk * 32);
#pragma unroll
    for (int tt = 0; tt < NT; ++tt) {
        const int j0 = (w + Q1_WAVES * tt) * 16;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < NK; ++kk) acc = mfma16(a[tt][kk], b[kk], acc);
        if (ql < Q1_H) {                                  // D[reg i]: token j0 + 4 g + i, head ql
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int j = j0 + 4 * g + i;
                if (j < S) out[j * Q1_H + ql] = acc[i] * mul;
            }
        }
    }
}

// the wave's tokens w, w + 8, ... as feature slices (lane l: features 8 l ..)
__device__ __forceinline__ void q1_load_slices(const bf16_t* __restrict__ X, int S, int w, int lane, bf16x8 (&xr)[Q1_SLOTS]) {
#pragma unroll
    for (int t = 0; t < Q1_SLOTS; ++t) {
        const int j = min(w + Q1_WAVES * t, S - 1);       // clamped, not predicated: slots past the row are never used
        xr[t] = *(const bf16x8*)(X + (size_t)j * Q1_D + lane * 8);
    }
}

// acc[h][e] = sum over the wave's tokens j of coef[j][h] * x_j[8 lane + e]
__device__ __forceinline__ void q1_token_sums(const bf16x8 (&xr)[Q1_SLOTS], const float* coef, int S, int w, float (&acc)[Q1_H][8]) {
#pragma unroll
    for (int h = 0; h < Q1_H; ++h)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[h][e] = 0.f;
#pragma unroll
    for (int t = 0; t < Q1_SLOTS; ++t) {
        const int j = w + Q1_WAVES * t;
        if (j < S) {                                      // wave-uniform
            const f32x4 c0 = *(const f32x4*)(coef + j * Q1_H), c1 = *(const f32x4*)(coef + j * Q1_H + 4);
            float x[8];
            q1_unpack(xr[t], x);
#pragma unroll
            for (int h = 0; h < 4; ++h)
#pragma unroll
                for (int e = 0; e < 8; ++e) { acc[h][e] += c0[h] * x[e]; acc[h + 4][e] += c1[h] * x[e]; }
        }
    }
}

__device__ __forceinline__ void q1_red_store(const float (&acc)[Q1_H][8], float* buf, int lane) {
#pragma unroll
    for (int h = 0; h < Q1_H; ++h) {
        *(f32x4*)(buf + h * Q1_D + lane * 8) = f32x4{acc[h][0], acc[h][1], acc[h][2], acc[h][3]};
        *(f32x4*)(buf + h * Q1_D + lane * 8 + 4) = f32x4{acc[h][4], acc[h][5], acc[h][6], acc[h][7]};
    }
}
__device__ __forceinline__ void q1_red_add(float (&acc)[Q1_H][8], const float* buf, int lane) {
#pragma unroll
    for (int h = 0; h < Q1_H; ++h) {
        const f32x4 a = *(const f32x4*)(buf + h * Q1_D + lane * 8), b = *(const f32x4*)(buf + h * Q1_D + lane * 8 + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { acc[h][e] += a[e]; acc[h][e + 4] += b[e]; }
    }
}
// sum of the 8 waves' partials -> out[8, 512] bf16, written by wave 0.  red: 4 buffers of Q1_RED_FLOATS; a wave only ever overwrites a buffer that it alone has read.
__device__ __forceinline__ void q1_reduce_write(float (&acc)[Q1_H][8], float* red, int w, int lane, bf16_t* __restrict__ out) {
    if (w >= 4) q1_red_store(acc, red + (w - 4) * Q1_RED_FLOATS, lane);
    __syncthreads();
    if (w < 4) q1_red_add(acc, red + w * Q1_RED_FLOATS, lane);
    if (w == 2 || w == 3) q1_red_store(acc, red + w * Q1_RED_FLOATS, lane);
    __syncthreads();
    if (w < 2) q1_red_add(acc, red + (w + 2) * Q1_RED_FLOATS, lane);
    if (w == 1) q1_red_store(acc, red + Q1_RED_FLOATS, lane);
    __syncthreads();
    if (w == 0) {
        q1_red_add(acc, red + Q1_RED_FLOATS, lane);
#pragma unroll
        for (int h = 0; h < Q1_H; ++h) *(bf16x8*)(out + h * Q1_D + lane * 8) = pack8(acc[h]);
    }
}

struct Q1Args {
    const bf16_t* X; long ldx;          // tokens: row r at X + r * ldx, [S, 512]
    const bf16_t* QT;                   // [R, 8, 512]
    bf16_t* C; float* SIG; float* P;    // forward outputs: [R, 8, 512], [R, 8], [R, 8, S]
    const bf16_t* DC; const float* DSIG;// backward inputs: [R, 8, 512], [R, 8]
    bf16_t* DX; long lddx; bf16_t* DQT; // backward outputs: [R, S, 512] with a row stride, [R, 8, 512]
    int S; float scale; DropCfg drop;
};

__global__ void __launch_bounds__(Q1_THREADS, 1) attn_q1_fwd_kernel(Q1Args p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* sc = (float*)smem;                          // [Q1_SMAX][8]: scores, then dropped-out probabilities
    float* red = sc + Q1_SMAX * Q1_H;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, S = p.S;      // w in an SGPR: its branches are scalar
    const size_t r = blockIdx.x;
    const DropCfg drop = drop_resolve(p.drop);
    const bf16_t* X = p.X + r * p.ldx;
    q1_token_head_products(X, p.QT + r * (Q1_H * Q1_D), S, p.scale, sc, w, lane);      // the HBM read (its registers are free again before the slices land)
    bf16x8 xr[Q1_SLOTS];
    q1_load_slices(X, S, w, lane, xr);                 // the same lines again, from L2
    __syncthreads();
    {   // wave w = head w
        const int h = w;
        float v[Q1_SMAX / 64], m = -INFINITY, sum = 0.f, sig = 0.f;
#pragma unroll
        for (int i = 0; i < Q1_SMAX / 64; ++i) {
            const int j = lane + 64 * i;
            v[i] = j < S ? sc[j * Q1_H + h] : -INFINITY;
            m = fmaxf(m, v[i]);
        }
        m = wave_max(m);
#pragma unroll
        for (int i = 0; i < Q1_SMAX / 64; ++i) { v[i] = __expf(v[i] - m); sum += v[i]; }      // keys >= S: exp(-inf) = 0
        const float inv = 1.f / wave_sum(sum);
        const unsigned long long e0 = att_drop_row(S, Q1_H, (int)r, h, 0);
#pragma unroll
        for (int i = 0; i < Q1_SMAX / 64; ++i) {
            const int j = lane + 64 * i;
            if (j < S) {
                const float pr = v[i] * inv;
                const float pd = (!drop.thr || att_keep1(drop, e0 + j)) ? pr * drop.scale : 0.f;
                p.P[(r * Q1_H + h) * S + j] = pr;
                sc[j * Q1_H + h] = pd;
                sig += pd;
            }
        }
        sig = wave_sum(sig);
        if (lane == 0) p.SIG[r * Q1_H + h] = sig;
    }
    __syncthreads();
    float acc[Q1_H][8];
    q1_token_sums(xr, sc, S, w, acc);
    q1_reduce_write(acc, red, w, lane, p.C + r * (Q1_H * Q1_D));
}

__global__ void __launch_bounds__(Q1_THREADS, 1) attn_q1_bwd_kernel(Q1Args p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* dsb = (float*)smem;                         // [Q1_SMAX][8]: dpd = dc . x, then dS
    float* pdb = dsb + Q1_SMAX * Q1_H;                 // [Q1_SMAX][8]: dropped-out probabilities
    float* red = pdb + Q1_SMAX * Q1_H;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, S = p.S;      // w in an SGPR: its branches are scalar
    const size_t r = blockIdx.x;
    const DropCfg drop = drop_resolve(p.drop);
    const bf16_t* X = p.X + r * p.ldx;
    q1_token_head_products(X, p.DC + r * (Q1_H * Q1_D), S, 1.f, dsb, w, lane);
    bf16x8 xr[Q1_SLOTS];
    q1_load_slices(X, S, w, lane, xr);
    __syncthreads();
    {   // wave w = head w: dp = keep / (1 - p) * (dpd + dsigma), dS = scale * P * (dp - sum_i P_i dp_i)
        const int h = w;
        const float dsig = p.DSIG[r * Q1_H + h];
        const unsigned long long e0 = att_drop_row(S, Q1_H, (int)r, h, 0);
        float pr[Q1_SMAX / 64], dp[Q1_SMAX / 64], delta = 0.f;
#pragma unroll
        for (int i = 0; i < Q1_SMAX / 64; ++i) {
            const int j = lane + 64 * i;
            pr[i] = 0.f; dp[i] = 0.f;
            if (j < S) {
                pr[i] = p.P[(r * Q1_H + h) * S + j];
                const bool keep = !drop.thr || att_keep1(drop, e0 + j);
                dp[i] = keep ? (dsb[j * Q1_H + h] + dsig) * drop.scale : 0.f;
                pdb[j * Q1_H + h] = keep ? pr[i] * drop.scale : 0.f;
                delta += pr[i] * dp[i];
            }
        }
        delta = wave_sum(delta);
#pragma unroll
        for (int i = 0; i < Q1_SMAX / 64; ++i) {
            const int j = lane + 64 * i;
            if (j < S) dsb[j * Q1_H + h] = p.scale * pr[i] * (dp[i] - delta);
        }
    }
    __syncthreads();
    {
        float acc[Q1_H][8];
        q1_token_sums(xr, dsb, S, w, acc);                 // dqt_h = sum_j dS_hj x_j
        q1_reduce_write(acc, red, w, lane, p.DQT + r * (Q1_H * Q1_D));
    }
    // dx_j = sum_h dS_hj qt_h + pd_hj dc_h: every token of the row is written
    float qf[Q1_H][8], cf[Q1_H][8];
    const bf16_t* QT = p.QT + r * (Q1_H * Q1_D) + lane * 8;
    const bf16_t* DC = p.DC + r * (Q1_H * Q1_D) + lane * 8;
#pragma unroll
    for (int h = 0; h < Q1_H; ++h) {
        q1_unpack(*(const bf16x8*)(QT + h * Q1_D), qf[h]);
        q1_unpack(*(const bf16x8*)(DC + h * Q1_D), cf[h]);
    }
    bf16_t* DX = p.DX + r * p.lddx;
#pragma unroll 1
    for (int j = w; j < S; j += Q1_WAVES) {
        const f32x4 s0 = *(const f32x4*)(dsb + j * Q1_H), s1 = *(const f32x4*)(dsb + j * Q1_H + 4);
        const f32x4 d0 = *(const f32x4*)(pdb + j * Q1_H), d1 = *(const f32x4*)(pdb + j * Q1_H + 4);
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = 0.f;
#pragma unroll
        for (int h = 0; h < 4; ++h)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                o[e] += s0[h] * qf[h][e] + d0[h] * cf[h][e];
                o[e] += s1[h] * qf[h + 4][e] + d1[h] * cf[h + 4][e];
            }
        *(bf16x8*)(DX + (size_t)j * Q1_D + lane * 8) = pack8(o);
    }
}

static bool q1_shape_ok(int R, int S, long ldx) { return R > 0 && S > 0 && S <= Q1_SMAX && ldx >= (long)S * Q1_D && ldx % 8 == 0; }

extern "C" int svla_attn_q1_fwd_bf16(const bf16_t* X, long ldx, const bf16_t* QT, bf16_t* C, float* SIG, float* P, int R, int S, float scale,
                                     const svla_dropout* drop, void* stream) {
    if (!X || !QT || !C || !SIG || !P || !q1_shape_ok(R, S, ldx)) return SVLA_EINVAL;
    Q1Args p{};
    p.X = X; p.ldx = ldx; p.QT = QT; p.C = C; p.SIG = SIG; p.P = P; p.S = S; p.scale = scale; p.drop = drop_cfg(drop);
    return svla_launch<attn_q1_fwd_kernel>(dim3(R), dim3(Q1_THREADS), Q1_LDS_FWD, (hipStream_t)stream, p);
}

extern "C" int svla_attn_q1_bwd_bf16(const bf16_t* X, long ldx, const bf16_t* QT, const bf16_t* DC, const float* DSIG, const float* P,
                                     bf16_t* DX, long lddx, bf16_t* DQT, int R, int S, float scale, const svla_dropout* drop, void* stream) {
    if (!X || !QT || !DC || !DSIG || !P || !DX || !DQT || !q1_shape_ok(R, S, ldx) || !q1_shape_ok(R, S, lddx)) return SVLA_EINVAL;
    Q1Args p{};
    p.X = X; p.ldx = ldx; p.QT = QT; p.DC = DC; p.DSIG = DSIG; p.P = (float*)P; p.DX = DX; p.lddx = lddx; p.DQT = DQT;
    p.S = S; p.scale = scale; p.drop = drop_cfg(drop);
    return svla_launch<attn_q1_bwd_kernel>(dim3(R), dim3(Q1_THREADS), Q1_LDS_BWD, (hipStream_t)stream, p);
}

// ---- head-expanded operands: row r * 8 + h of E holds v[r] with the columns outside head h's 64 zeroed, so a plain [8 R, 512] x [512, 512] GEMM applies
// head h's 64-row block of a weight to head h's slice only.  One wave per source row; lane l holds columns 8 l .. 8 l + 7 (head l >> 3).
//   dot (optional, with bias):   dot[r, h] = sum_d v[r, 64 h + d] * bias[64 h + d]          (dsigma_h = do_h . b_v,h)
//   vs  (optional, with sigma):  vs[r, 64 h + d] = sigma[r, h] * v[r, 64 h + d]             (rows whose column sum is db_v)
__global__ void __launch_bounds__(256) head_expand_kernel(const bf16_t* __restrict__ v, long ldv, int R, bf16_t* __restrict__ E, const float* __restrict__ bias,
                                                          float* __restrict__ dot, const float* __restrict__ sigma, bf16_t* __restrict__ vs) {
    const size_t r = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, hl = lane >> 3;
    if (r >= (size_t)R) return;
    const bf16x8 x = *(const bf16x8*)(v + r * ldv + lane * 8);
    const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int h = 0; h < Q1_H; ++h) *(bf16x8*)(E + (r * Q1_H + h) * Q1_D + lane * 8) = h == hl ? x : z;
    if (!bias && !sigma) return;
    float f[8];
    q1_unpack(x, f);
    if (bias) {
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) s += f[e] * bias[lane * 8 + e];
        s += __shfl_xor(s, 1, 64); s += __shfl_xor(s, 2, 64); s += __shfl_xor(s, 4, 64);
        if ((lane & 7) == 0) dot[r * Q1_H + hl] = s;
    }
    if (sigma) {
        const float sg = sigma[r * Q1_H + hl];
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] *= sg;
        *(bf16x8*)(vs + r * Q1_D + lane * 8) = pack8(f);
    }
}
// out[r, 64 h + d] = G[r * 8 + h, 64 h + d] (+ sigma[r, h] * bias[64 h + d]): the diagonal 64-wide blocks of a product over head-expanded rows
__global__ void __launch_bounds__(256) head_pick_kernel(const bf16_t* __restrict__ G, int R, const float* __restrict__ sigma, const float* __restrict__ bias,
                                                        bf16_t* __restrict__ out, long ldo) {
    const size_t r = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, hl = lane >> 3;
    if (r >= (size_t)R) return;
    bf16x8 x = *(const bf16x8*)(G + (r * Q1_H + hl) * Q1_D + lane * 8);
    if (sigma) {
        float f[8];
        q1_unpack(x, f);
        const float sg = sigma[r * Q1_H + hl];
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] += sg * bias[lane * 8 + e];
        x = pack8(f);
    }
    *(bf16x8*)(out + r * ldo + lane * 8) = x;
}

extern "C" int svla_head_expand_bf16(const bf16_t* v, long ldv, int R, bf16_t* E, const float* bias, float* dot, const float* sigma, bf16_t* vs, void* stream) {
    if (!v || !E || R <= 0 || ldv < Q1_D || ldv % 8 || (bias && !dot) || (sigma && !vs)) return SVLA_EINVAL;
    return svla_launch<head_expand_kernel>(dim3((R + 3) / 4), dim3(256), 0, (hipStream_t)stream, v, ldv, R, E, bias, dot, sigma, vs);
}
extern "C" int svla_head_pick_bf16(const bf16_t* G, int R, const float* sigma, const float* bias, bf16_t* out, long ldo, void* stream) {
    if (!G || !out || R <= 0 || ldo < Q1_D || ldo % 8 || (sigma && !bias)) return SVLA_EINVAL;
    return svla_launch<head_pick_kernel>(dim3((R + 3) / 4), dim3(256), 0, (hipStream_t)stream, G, R, sigma, bias, out, ldo);
}
