// Antialiased bicubic resize of uint8 camera frames: the torchvision Resize(size, bicubic, antialias=True) that tensor_image_preprocessor prepends when the model's
// input size is not the camera's (architecture/models/transformer_models/preprocessors.py:35-43; 224 x 384 -> 256 x 256 for the SigLIP trunk), u8 [B,H,W,3] ->
// u8 [B,OH,OW,3] in one launch.
//
// Arithmetic contract: that of F.interpolate(x.float(), mode="bicubic", antialias=True, align_corners=False) -> clamp(0, 255) -> round half to even ->
// u8.  Per axis, scale = in / out, s = max(scale, 1), support = 2 s, centre = scale (i + 0.5): taps j in [max(0, int(centre - support + 0.5)),
// min(in, int(centre + support + 0.5))), weights cubic((j - centre + 0.5) / s) with a = -0.5 (Keys) divided by their sum.  Horizontal pass first, then vertical; the
// intermediate is fp32 and is not rounded.  Equal sizes: the weights collapse to (0, 1, 0, 0), an exact copy.
//
// One block makes a TR x TC tile of the output: the source rectangle of the tile is staged as bytes (aligned dwords of the HWC stream, as csrc/augment.hip does), the
// horizontal pass writes fp32 rows [source row][tile column * 3] to LDS, the vertical pass reads them and stores dwords.  Tap positions and weights are computed in
// the kernel, in fp64, once per tile row / column.  The tile shape and the LDS sizes depend on the geometry only; the host finds them with the same span function.
#include "common.h"
#pragma clang fp contract(off)      // the host sizes the LDS rectangles with rsz_span: host and device must round it alike

#define RSZ_T 256
#define RSZ_LDS_MAX (48 * 1024)

// source taps [j0, j1) of output index i
__host__ __device__ inline void rsz_span(int i, double scale, int in, int& j0, int& j1) {
    const double support = 2.0 * (scale > 1.0 ? scale : 1.0), centre = scale * ((double)i + 0.5);
    j0 = (int)(centre - support + 0.5);
    j0 = j0 < 0 ? 0 : j0;
    j1 = (int)(centre + support + 0.5);
    j1 = j1 > in ? in : j1;
}
__device__ __forceinline__ double rsz_cubic(double x) {      // Keys, a = -0.5
    x = fabs(x);
    if (x < 1.0) return ((1.5 * x - 2.5) * x) * x + 1.0;
    if (x < 2.0) return ((-0.5 * x + 2.5) * x - 4.0) * x + 2.0;
    return 0.0;
}
// first tap and the K normalised weights (zero past the index's own taps) of output index i -> j0, w[k * stride]
__device__ __forceinline__ void rsz_taps(int i, double scale, int in, int K, int& j0, float* w, int stride) {
    int j1;
    rsz_span(i, scale, in, j0, j1);
    const int n = min(j1 - j0, K);
    const double s = scale > 1.0 ? scale : 1.0, centre = scale * ((double)i + 0.5);
    double tot = 0.0;
    for (int k = 0; k < n; ++k) tot += rsz_cubic(((double)(j0 + k) - centre + 0.5) / s);
    for (int k = 0; k < K; ++k) w[k * stride] = k < n ? (float)(rsz_cubic(((double)(j0 + k) - centre + 0.5) / s) / tot) : 0.f;
}
__device__ __forceinline__ unsigned rsz_round_u8(float v) { return (unsigned)rintf(fminf(fmaxf(v, 0.f), 255.f)); }      // clamp, round half to even

struct RszGeom { int H, W, OH, OW, TR, TC, Ky, Kx, nrcap, nccap; double sy, sx; };
__host__ __device__ inline int rsz_pitch(int nccap) { return ((nccap * 3 + 3) & ~3) + 8; }      // staged row: 0..3 lead bytes + nccap pixels, whole dwords
__host__ __device__ inline size_t rsz_lds_bytes(const RszGeom& g) {
    return (size_t)4 * (g.Kx * g.TC + g.Ky * g.TR + g.TC + g.TR) + (size_t)4 * g.nrcap * g.TC * 3 + (size_t)g.nrcap * rsz_pitch(g.nccap) + (size_t)((g.nrcap + 3) & ~3);
}

// grid (tiles, B), TC in {16, 32, 64, 128} (RSZ_T / TC rows of the horizontal pass per sweep), TR % 4 == 0, TC + TR <= RSZ_T
__global__ void __launch_bounds__(RSZ_T) resize_bicubic_aa_u8_kernel(const unsigned char* __restrict__ x, unsigned char* __restrict__ y, RszGeom G,
                                                                     const unsigned char* tb, const unsigned char* te) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int TR = G.TR, TC = G.TC, Kx = G.Kx, Ky = G.Ky, MP = TC * 3;
    float* wx = (float*)smem;                        // [Kx][TC]
    float* wy = wx + Kx * TC;                        // [Ky][TR]
    int* x0s = (int*)(wy + Ky * TR);                 // [TC] first tap of a tile column
    int* y0s = x0s + TC;                             // [TR] first tap of a tile row
    float* mid = (float*)(y0s + TR);                 // [nrcap][TC * 3]: the horizontal pass, 16-byte aligned rows
    unsigned char* in = (unsigned char*)(mid + (size_t)G.nrcap * MP);      // [nrcap][pitch] staged source bytes
    const int pitch = rsz_pitch(G.nccap);
    unsigned char* leads = in + (size_t)G.nrcap * pitch;
    const int t = threadIdx.x;
    const int tilesx = (G.OW + TC - 1) / TC;
    const int tx = blockIdx.x % tilesx, ty = blockIdx.x / tilesx, b = blockIdx.y;
    const int ox0 = tx * TC, oy0 = ty * TR;
    const int tw = min(TC, G.OW - ox0), th = min(TR, G.OH - oy0);
    int xa, xb, ya, yb, tmp;
    rsz_span(ox0, G.sx, G.W, xa, tmp);
    rsz_span(ox0 + tw - 1, G.sx, G.W, tmp, xb);
    rsz_span(oy0, G.sy, G.H, ya, tmp);
    rsz_span(oy0 + th - 1, G.sy, G.H, tmp, yb);
    const int nrin = min(yb - ya, G.nrcap), ncin = min(xb - xa, G.nccap);      // the host sized the caps with the same function: the min never bites
    if (t < tw) rsz_taps(ox0 + t, G.sx, G.W, Kx, x0s[t], wx + t, TC);
    else if (t >= TC && t - TC < th) rsz_taps(oy0 + t - TC, G.sy, G.H, Ky, y0s[t - TC], wy + (t - TC), TR);
    // ---- source rectangle -> LDS bytes: aligned dwords; a dword that is not wholly inside the tensor [tb, te) is assembled from its bytes that are
    const size_t RB = (size_t)G.W * 3;
    const unsigned char* img = x + (size_t)b * G.H * RB + (size_t)ya * RB + (size_t)xa * 3;
    const int nb = ncin * 3, ndw = (nb + 6) / 4;
    for (int i = t; i < nrin * ndw; i += RSZ_T) {
        const int r = i / ndw, j = i - r * ndw;
        const unsigned char* g = img + (size_t)r * RB;
        const int lead = (int)((uintptr_t)g & 3);
        if (j == 0) leads[r] = (unsigned char)lead;
        if (4 * j >= lead + nb) continue;
        const unsigned char* a = g - lead + 4 * j;
        uint32_t w = 0;
        if (a >= tb && a + 4 <= te) w = *(const uint32_t*)a;
        else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (a + e >= tb && a + e < te) w |= (uint32_t)a[e] << (8 * e);
        }
        *(uint32_t*)(in + (size_t)r * pitch + 4 * j) = w;
    }
    __syncthreads();
    // ---- horizontal pass: thread = one tile column, RSZ_T / TC source rows per sweep
    {
        const int c = t & (TC - 1), rstep = RSZ_T / TC;
        if (c < tw) {
            const int cx = x0s[c] - xa;
            for (int r = t / TC; r < nrin; r += rstep) {
                const unsigned char* p = in + (size_t)r * pitch + leads[r];
                float a0 = 0.f, a1 = 0.f, a2 = 0.f;
                for (int k = 0; k < Kx; ++k) {
                    const float w = wx[k * TC + c];
                    const unsigned char* q = p + min(cx + k, ncin - 1) * 3;      // past the column's own taps the weight is 0
                    a0 += w * (float)q[0]; a1 += w * (float)q[1]; a2 += w * (float)q[2];
                }
                float* m = mid + (size_t)r * MP + c * 3;
                m[0] = a0; m[1] = a1; m[2] = a2;
            }
        }
    }
    __syncthreads();
    // ---- vertical pass + store: aligned dwords inside a row segment, its 0..3 head / tail bytes as bytes
    const int nbo = tw * 3, ndwo = (nbo + 6) / 4;
    unsigned char* yimg = y + ((size_t)b * G.OH + oy0) * G.OW * 3 + (size_t)ox0 * 3;
    for (int i = t; i < th * ndwo; i += RSZ_T) {
        const int r = i / ndwo, j = i - r * ndwo;
        unsigned char* g = yimg + (size_t)r * G.OW * 3;
        const int lead = (int)((uintptr_t)g & 3);
        if (4 * j >= lead + nbo) continue;
        const int lo = 4 * j - lead, ry = y0s[r] - ya;
        if (lo >= 0 && lo + 4 <= nbo) {
            float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
            if (lead == 0) {      // the usual case (OW * 3 and the frame base are multiples of 4): one 16-byte LDS read per tap
                for (int k = 0; k < Ky; ++k) {
                    const float w = wy[k * TR + r];
                    const f32x4 m = *(const f32x4*)(mid + (size_t)min(ry + k, nrin - 1) * MP + lo);
                    v0 += w * m[0]; v1 += w * m[1]; v2 += w * m[2]; v3 += w * m[3];
                }
            } else {
                for (int k = 0; k < Ky; ++k) {
                    const float w = wy[k * TR + r];
                    const float* m = mid + (size_t)min(ry + k, nrin - 1) * MP + lo;
                    v0 += w * m[0]; v1 += w * m[1]; v2 += w * m[2]; v3 += w * m[3];
                }
            }
            *(uint32_t*)(g + lo) = rsz_round_u8(v0) | (rsz_round_u8(v1) << 8) | (rsz_round_u8(v2) << 16) | (rsz_round_u8(v3) << 24);
        } else {
            for (int e = 0; e < 4; ++e) {
                const int kb = lo + e;
                if (kb < 0 || kb >= nbo) continue;
                float v = 0.f;
                for (int k = 0; k < Ky; ++k) v += wy[k * TR + r] * mid[(size_t)min(ry + k, nrin - 1) * MP + kb];
                g[kb] = (unsigned char)rsz_round_u8(v);
            }
        }
    }
}

// ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
// largest tap count of an axis, and the longest source span of a tile of T output indices
static void rsz_axis(int in, int out, double scale, int T, int& K, int& cap) {
    K = 0; cap = 0;
    for (int i = 0; i < out; ++i) {
        int j0, j1;
        rsz_span(i, scale, in, j0, j1);
        K = j1 - j0 > K ? j1 - j0 : K;
    }
    for (int i0 = 0; i0 < out; i0 += T) {
        int j0, j1, tmp;
        rsz_span(i0, scale, in, j0, tmp);
        rsz_span((i0 + T < out ? i0 + T : out) - 1, scale, in, tmp, j1);
        cap = j1 - j0 > cap ? j1 - j0 : cap;
    }
}

extern "C" int svla_resize_bicubic_aa_u8(const unsigned char* x, unsigned char* y, int B, int H, int W, int OH, int OW, void* stream) {
    if (!x || !y || x == y || B < 1 || B > 65535 || H < 4 || W < 4 || OH < 4 || OW < 4) return SVLA_EINVAL;
    if ((long long)H > 4ll * OH || (long long)OH > 4ll * H || (long long)W > 4ll * OW || (long long)OW > 4ll * W) return SVLA_EINVAL;      // per-axis scale in [1/4, 4]
    if ((long long)H * W * 3 >= (1ll << 31) || (long long)OH * OW * 3 >= (1ll << 31)) return SVLA_EINVAL;
    RszGeom G{H, W, OH, OW, 32, 64, 0, 0, 0, 0, (double)H / (double)OH, (double)W / (double)OW};
    for (;;) {      // the largest tile whose source rectangle and fp32 rows fit: 32 x 64 at the camera's ratios, 4 x 64 at scale 4 on both axes
        rsz_axis(H, OH, G.sy, G.TR, G.Ky, G.nrcap);
        rsz_axis(W, OW, G.sx, G.TC, G.Kx, G.nccap);
        if (rsz_lds_bytes(G) <= RSZ_LDS_MAX) break;
        if (G.TR > 4) G.TR /= 2;
        else if (G.TC > 16) G.TC /= 2;
        else return SVLA_EINVAL;
    }
    const long long tiles = (long long)((OH + G.TR - 1) / G.TR) * ((OW + G.TC - 1) / G.TC);
    if (tiles >= (1ll << 31)) return SVLA_EINVAL;
    return svla_launch<resize_bicubic_aa_u8_kernel>(dim3((unsigned)tiles, B), dim3(RSZ_T), rsz_lds_bytes(G), (hipStream_t)stream, x, y, G, x,
                       x + (size_t)B * H * W * 3);
}
