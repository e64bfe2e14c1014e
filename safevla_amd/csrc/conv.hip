// Convolutions of the frozen CLIP RN50 image trunk (architecture/models/transformer_models/image_encoders.py:11-48 runs CLIP's ModifiedResNet, layers (3, 4, 6, 3),
// width 64, on 224 x 384 frames; preprocessing architecture/models/transformer_models/preprocessors.py:27).  Activations are NHWC bf16 = rows [B*H*W, C], the
// layout of the GEMMs and of the token tensors.  Three kernels:
//   conv_igemm_bf16_kernel<BN>   3x3 (stride 1, pad 1) and 1x1 convolutions as an implicit GEMM on v_mfma_f32_16x16x32_bf16, fp32 accumulation
//   conv_stem_u8_bf16_kernel     u8 frame -> normalise -> 3x3 stride-2 conv (3 -> 32) -> folded BN -> ReLU, one streaming pass (K = 27 is too thin for MFMA)
//   avgpool2_nhwc_bf16_kernel    AvgPool2d(2), floor semantics, fp32 sum
// BatchNorm (eval) is folded on the host: the weights carry gamma / sqrt(var + eps), the fp32 bias the shift.
//
// ---- the implicit GEMM ------------------------------------------------------------------------------------------------------------
// M = B*H*W output pixels, N = Cout, K = taps*Cin with k = tap*Cin + c: weights [Cout, taps, Cin] are K-major rows, and for one tap the 32 channels of a k-step are
// 64 contiguous bytes of one input pixel.  No im2col matrix exists anywhere: the A operand of k-step (tap, c0) is gathered from x at pixel + (dy*W + dx), and a
// neighbour outside the image -- across a row end, the image's first / last row or the next image of the batch -- is a zero in the register, decided per output
// pixel from its own (oy, ox): a tile of 128 consecutive pixels may span any number of rows and images (any H, W >= 1).
//
// Tile: 128 pixels x BN channels per 256-thread block (BN = 128 / 64 / 32, the largest that divides Cout), k-step 32 (the smallest Cin), four waves as 2 (pixels) x 2
// (channels), a wave owns 64 pixels x BN/2 channels = 4 x BN/32 accumulators of 16 x 16.  The MFMA computes the TRANSPOSED tile, D = W . X^T (weights as the A
// operand, pixels as the B operand -- both fragments have the same lane map, row l & 15, k = 8 (l >> 4) + 0..7): the result has the pixel on the lane (l & 15) and four
// consecutive channels 4 (l >> 4) + 0..3 in the lane's registers, so the epilogue packs them into one 8-byte store (the untransposed product would leave 2-byte stores).
//
// Both operands go through LDS (choice and reason in DESIGN.md 4f: every gathered pixel row is read by both channel-waves and every weight row by both pixel-waves; read
// straight into fragments the block would fetch each twice through the vector L1).  Two buffers, one barrier per k-step: the loads of step s + 1 are issued
// before the MFMAs of step s and written to the other buffer after them.
//
// LDS image of one operand tile: rows of 32 bf16 = 64 bytes = four 16-byte slots, no padding; slot q of row r is stored at slot position q ^ g(r), g(r) = (0 - (r >> 2)) & 3.
//   * fragment read: ds_read_b128, lane l reads slot q = l >> 4 of row (l & 15) of a 16-row sub-tile.  The LDS serves a b128 read in four groups of 16 lanes, and the
//     groups are NOT the quarter-waves: group 0 = lanes {0-3, 12-15, 20-27} = rows {0-3, 12-15} at q = 0 and rows {4-11} at q = 1 (MI355X LDS table).  A 256-byte bank
//     row holds four 64-byte rows, so rows r and r + 4 meet on the same banks unless their slot positions differ: for the row quads 0, 3 (q = 0) and 1, 2 (q = 1) of
//     group 0 the positions are g(0) = 0, g(3) = 1, 1 ^ g(1) = 2, 1 ^ g(2) = 3 -- four different slots in each of the four 64-byte lanes of the bank row: conflict-free.
//     Group 1 (row quads 1, 2 at q = 0; 0, 3 at q = 1): 3, 2, 1, 0.  Groups 2, 3 are groups 0, 1 with q ^ 2.  (The textbook g = r >> 2 fails here: 1 ^ g(1) = g(0).)
//   * fill: ds_write_b128, thread t writes slot t & 3 of row t >> 2: eight consecutive lanes (the write's service group) cover two whole rows = 128 contiguous bytes,
//     permuted inside each row: all 32 banks once.
// LDS per block: 2 buffers x (128 + BN) rows x 64 bytes = 32 / 24 / 20 KiB.
#include "common.h"

#define CV_BM 128
#define CV_BK 32
#define CV_T 256

enum { CV_EPI_BIAS = 0, CV_EPI_RELU = 1, CV_EPI_RES_RELU = 2 };

struct ConvArgs {
    const bf16_t* x; const bf16_t* w; const float* bias; const bf16_t* res; long ldr;
    bf16_t* y; long ldy; int yG; long yGS;
    int M, H, W, Cin, Cout, taps, epi;
};

// element offset of 16-byte slot q of row r in a [rows][32] bf16 tile
__device__ __forceinline__ int cv_slot(int r, int q) { return r * CV_BK + ((q ^ ((0 - (r >> 2)) & 3)) << 3); }

template <int BN>
__global__ void __launch_bounds__(CV_T, 2) conv_igemm_bf16_kernel(ConvArgs p) {
    constexpr int NT = BN / 32;                                   // 16-channel sub-tiles per wave
    constexpr int TILE = (CV_BM + BN) * CV_BK;                    // bf16 elements of one buffer: pixel rows, then weight rows
    constexpr int NB = (BN * 4 + CV_T - 1) / CV_T;                // weight slots per thread (BN = 32: the first two waves load one each)
    __shared__ __attribute__((aligned(16))) bf16_t lds[2 * TILE];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int nt = p.Cout / BN;
    const int n0 = ((int)blockIdx.x % nt) * BN, m0 = ((int)blockIdx.x / nt) * CV_BM;      // the channel tiles of one pixel tile are neighbours in launch order
    const int H = p.H, W = p.W, Cin = p.Cin;
    const long K = (long)p.taps * Cin;

    // ---- what this thread stages: slot sq of pixel rows (t >> 2) and (t >> 2) + 64; slot sq of weight rows (t >> 2) (+ 64)
    const int sq = t & 3, sr = t >> 2;
    int oy[2], ox[2];
    const bf16_t* xp[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = m0 + sr + 64 * i;
        const int rem = m % (H * W);
        oy[i] = m < p.M ? rem / W : -4;                           // a row past M: every tap falls outside
        ox[i] = rem % W;
        xp[i] = p.x + (long)m * Cin + 8 * sq;
    }
    const bf16_t* wp = p.w + (long)(n0 + sr) * K + 8 * sq;

    u32x4 ra[2], rb[NB];
    auto load_step = [&](int tap, int c0) {
        const int dy = p.taps == 9 ? tap / 3 - 1 : 0, dx = p.taps == 9 ? tap % 3 - 1 : 0;
        const long shift = ((long)dy * W + dx) * Cin + c0;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const bool ok = (unsigned)(oy[i] + dy) < (unsigned)H && (unsigned)(ox[i] + dx) < (unsigned)W;
            const bf16_t* src = ok ? xp[i] + shift : p.x;         // always a readable address: the load is unconditional, the border is a select
            const u32x4 v = *(const u32x4*)src;
            ra[i] = ok ? v : u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int j = 0; j < NB; ++j)
            if (BN * 4 >= CV_T * (j + 1) || t < BN * 4 - CV_T * j) rb[j] = *(const u32x4*)(wp + (long)(64 * j) * K + (long)tap * Cin + c0);
    };
    auto store_step = [&](bf16_t* buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) *(u32x4*)(buf + cv_slot(sr + 64 * i, sq)) = ra[i];
#pragma unroll
        for (int j = 0; j < NB; ++j)
            if (BN * 4 >= CV_T * (j + 1) || t < BN * 4 - CV_T * j) *(u32x4*)(buf + CV_BM * CV_BK + cv_slot(sr + 64 * j, sq)) = rb[j];
    };

    const int wm = wave >> 1, wn = wave & 1, fr = lane & 15, fq = lane >> 4;
    f32x4 acc[NT][4];
#pragma unroll
    for (int ni = 0; ni < NT; ++ni)
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) acc[ni][mi] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nsteps = p.taps * (Cin / CV_BK);
    int tap = 0, c0 = 0;
    load_step(0, 0);
    store_step(lds);
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
        const bf16_t* cur = lds + (s & 1) * TILE;
        const bool more = s + 1 < nsteps;
        if (more) {
            c0 += CV_BK;
            if (c0 == Cin) { c0 = 0; ++tap; }
            load_step(tap, c0);
        }
        bf16x8 xf[4], wf[NT];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) xf[mi] = *(const bf16x8*)(cur + cv_slot(wm * 64 + mi * 16 + fr, fq));
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) wf[ni] = *(const bf16x8*)(cur + CV_BM * CV_BK + cv_slot(wn * (BN / 2) + ni * 16 + fr, fq));
#pragma unroll
        for (int ni = 0; ni < NT; ++ni)
#pragma unroll
            for (int mi = 0; mi < 4; ++mi) acc[ni][mi] = mfma16(wf[ni], xf[mi], acc[ni][mi]);      // D[channel 4 fq + reg][pixel fr]
        if (more) store_step(lds + ((s + 1) & 1) * TILE);
        __syncthreads();
    }

    // ---- epilogue: + bias [+ identity] [ReLU], four channels of one pixel per lane and sub-tile
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
        const int m = m0 + wm * 64 + mi * 16 + fr;
        if (m >= p.M) continue;
        const long orow = p.yG > 0 ? (long)(m / p.yG) * p.yGS + (m % p.yG) : (long)m;
        bf16_t* yrow = p.y + orow * p.ldy;
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) {
            const int c = n0 + wn * (BN / 2) + ni * 16 + 4 * fq;
            const f32x4 b = *(const f32x4*)(p.bias + c);
            f32x4 v = acc[ni][mi] + b;
            if (p.epi == CV_EPI_RES_RELU) {
                const u32x2 r = *(const u32x2*)(p.res + (long)m * p.ldr + c);
                v[0] += bf_lo(r[0]); v[1] += bf_hi(r[0]); v[2] += bf_lo(r[1]); v[3] += bf_hi(r[1]);
            }
            if (p.epi != CV_EPI_BIAS) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
            *(u32x2*)(yrow + c) = u32x2{pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};
        }
    }
}

// ---- stem: u8 [B,H,W,3] -> bf16 [B,OH,OW,32], OH = ceil(H/2), OW = ceil(W/2) ----------------------------------------------------------
// One output pixel per thread, 32 fp32 accumulators.  The normalisation is one multiply-add per input byte, (x / 255 - mean) / std = x * sc + of with
// sc = 1 / (255 std), of = -mean / std; the zero padding is a zero of the NORMALISED image (the reference pads after the normalisation).  w is fp32 [27][32],
// k = (ky*3 + kx)*3 + c, with the BatchNorm scale folded in; the block keeps them in LDS (3456 bytes) and every lane reads the same address: broadcast reads.
// (Read from global memory with their lane-uniform index, the compiler hoists all 864 into scalar registers and spills 806 of them.)
__global__ void __launch_bounds__(CV_T) conv_stem_u8_bf16_kernel(const unsigned char* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                                 bf16_t* __restrict__ y, long npix, int H, int W, int OH, int OW, float sc0, float sc1, float sc2,
                                                                 float of0, float of1, float of2) {
    __shared__ __attribute__((aligned(16))) float wl[27 * 32];
    for (int k = threadIdx.x; k < 27 * 32; k += CV_T) wl[k] = w[k];
    __syncthreads();
    const long i = (long)blockIdx.x * CV_T + threadIdx.x;
    if (i >= npix) return;
    const int ox = (int)(i % OW);
    const long q = i / OW;
    const int oy = (int)(q % OH);
    const long b = q / OH;
    const unsigned char* img = x + b * (long)H * W * 3;
    const float sc[3] = {sc0, sc1, sc2}, of[3] = {of0, of1, of2};
    float acc[32];
#pragma unroll
    for (int c = 0; c < 32; ++c) acc[c] = bias[c];
#pragma unroll 1                                                    // one tap's 96 weights at a time (unrolled, the compiler fetches all 864 first and spills)
    for (int tp = 0; tp < 9; ++tp) {
        const int iy = 2 * oy + tp / 3 - 1, ix = 2 * ox + tp % 3 - 1;
        const bool ok = (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
        const unsigned char* px = img + (ok ? ((long)iy * W + ix) * 3 : 0);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float v = ok ? (float)px[ch] * sc[ch] + of[ch] : 0.f;
            const f32x4* wk = (const f32x4*)(wl + (tp * 3 + ch) * 32);
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                const f32x4 w4 = wk[g];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[4 * g + e] += v * w4[e];
            }
        }
    }
    u32x4* out = (u32x4*)(y + i * 32);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        u32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = pack_bf2(fmaxf(acc[8 * g + 2 * e], 0.f), fmaxf(acc[8 * g + 2 * e + 1], 0.f));
        out[g] = o;
    }
}

// ---- AvgPool2d(2) on NHWC bf16: [B,H,W,C] -> [B,H/2,W/2,C] (floor: an odd last row / column is dropped), eight channels per thread, fp32 sum ----------------
__global__ void __launch_bounds__(CV_T) avgpool2_nhwc_bf16_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y, long n8, int H, int W, int C8) {
    const long i = (long)blockIdx.x * CV_T + threadIdx.x;
    if (i >= n8) return;
    const int OH = H / 2, OW = W / 2;
    const int c8 = (int)(i % C8);
    long q = i / C8;
    const int ox = (int)(q % OW); q /= OW;
    const int oy = (int)(q % OH);
    const long b = q / OH;
    const u32x4* src = (const u32x4*)x + ((b * H + 2 * oy) * W + 2 * ox) * C8 + c8;
    const u32x4 a = src[0], bq = src[C8], c = src[(long)W * C8], d = src[(long)W * C8 + C8];
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        o[e] = pack_bf2((bf_lo(a[e]) + bf_lo(bq[e]) + bf_lo(c[e]) + bf_lo(d[e])) * 0.25f, (bf_hi(a[e]) + bf_hi(bq[e]) + bf_hi(c[e]) + bf_hi(d[e])) * 0.25f);
    ((u32x4*)y)[i] = o;
}

// ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
static bool cv_aligned(const void* p, int a) { return p && ((uintptr_t)p % a) == 0; }

extern "C" int svla_conv_nhwc_bf16(const bf16_t* x, const bf16_t* w, const float* bias, const bf16_t* residual, long ldr, bf16_t* y, long ldy, int yG, long yGS,
                                   int B, int H, int W, int Cin, int Cout, int taps, int epi, void* stream) {
    if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || (Cin % 32) || (Cout % 32) || (taps != 1 && taps != 9)) return SVLA_EINVAL;
    if (epi < CV_EPI_BIAS || epi > CV_EPI_RES_RELU || ((epi == CV_EPI_RES_RELU) != (residual != nullptr))) return SVLA_EINVAL;
    if (!cv_aligned(x, 16) || !cv_aligned(w, 16) || !cv_aligned(bias, 16) || !cv_aligned(y, 8) || (residual && !cv_aligned(residual, 8))) return SVLA_EINVAL;
    if (ldy < Cout || (ldy % 4) || (residual && (ldr < Cout || (ldr % 4))) || yG < 0 || (yG > 0 && yGS < yG)) return SVLA_EINVAL;
    const long long M = (long long)B * H * W;
    if (M + CV_BM >= (1ll << 31)) return SVLA_EINVAL;
    const int BN = (Cout % 128) == 0 ? 128 : (Cout % 64) == 0 ? 64 : 32;
    const long long blocks = ((M + CV_BM - 1) / CV_BM) * (Cout / BN);
    if (blocks >= (1ll << 31)) return SVLA_EINVAL;
    ConvArgs p{x, w, bias, residual, ldr, y, ldy, yG, yGS, (int)M, H, W, Cin, Cout, taps, epi};
    const dim3 grid((unsigned)blocks), block(CV_T);
    if (BN == 128) return svla_launch<conv_igemm_bf16_kernel<128>>(grid, block, 0, (hipStream_t)stream, p);
    if (BN == 64) return svla_launch<conv_igemm_bf16_kernel<64>>(grid, block, 0, (hipStream_t)stream, p);
    return svla_launch<conv_igemm_bf16_kernel<32>>(grid, block, 0, (hipStream_t)stream, p);
}

extern "C" int svla_conv_stem_u8_bf16(const unsigned char* frames, int B, int H, int W, const float* mean3, const float* std3, const float* w, const float* bias,
                                      bf16_t* y, void* stream) {
    if (!frames || !mean3 || !std3 || !w || !bias || !cv_aligned(y, 16) || B <= 0 || H <= 0 || W <= 0) return SVLA_EINVAL;
    for (int c = 0; c < 3; ++c)
        if (!(std3[c] > 0.f)) return SVLA_EINVAL;
    const int OH = (H + 1) / 2, OW = (W + 1) / 2;
    const long long npix = (long long)B * OH * OW;
    if ((long long)B * H * W * 3 >= (1ll << 40) || (npix + CV_T - 1) / CV_T >= (1ll << 31)) return SVLA_EINVAL;
    float sc[3], of[3];
    for (int c = 0; c < 3; ++c) { sc[c] = 1.f / (255.f * std3[c]); of[c] = -mean3[c] / std3[c]; }
    return svla_launch<conv_stem_u8_bf16_kernel>(dim3((unsigned)((npix + CV_T - 1) / CV_T)), dim3(CV_T), 0, (hipStream_t)stream, frames, w, bias, y, (long)npix, H, W,
                       OH, OW, sc[0], sc[1], sc[2], of[0], of[1], of[2]);
}

extern "C" int svla_avgpool2_nhwc_bf16(const bf16_t* x, int B, int H, int W, int C, bf16_t* y, void* stream) {
    if (!cv_aligned(x, 16) || !cv_aligned(y, 16) || B <= 0 || H < 2 || W < 2 || C <= 0 || (C % 8)) return SVLA_EINVAL;
    const long long n8 = (long long)B * (H / 2) * (W / 2) * (C / 8);
    if ((n8 + CV_T - 1) / CV_T >= (1ll << 31)) return SVLA_EINVAL;
    return svla_launch<avgpool2_nhwc_bf16_kernel>(dim3((unsigned)((n8 + CV_T - 1) / CV_T)), dim3(CV_T), 0, (hipStream_t)stream, x, y, (long)n8, H, W, C / 8);
}
