// Frame augmentation of the camera preprocessors as u8 -> u8 kernels in front of svla_normalize_u8_f32 / svla_patchify_u8_bf16, in two launch forms:
//   * single-transform (architecture/allenact_preprocessors/dino_preprocessors.py:224-239 applies the transform that utils/transformation_util.py:54-119 samples
//     from the v2 list :12-28): one transform for the whole batch, its parameters are kernel arguments;
//   * grouped (the imitation-learning Preprocessor, architecture/models/transformer_models/preprocessors.py:86-118, applies the full random v2 list once per
//     trajectory and camera to that trajectory's [T, 3, H, W] frames, every call with newly drawn parameters; a batch [B, T, H, W, 3] therefore carries B
//     transforms): image n of the [N, H, W, 3] batch uses entry n / group_len of a [G] table of svla_aug_transform in device memory.
//
// Arithmetic contract (DESIGN.md "Sampled frame augmentation"): every stage takes and returns u8, every intermediate is rounded to u8 where the torchvision
// op list rounds it.  Three launches per camera per call, each stage stated ONCE as a device body that both launch forms call:
//   1. aug_gray_partials_body      integer partial sums of gray(x) per image, x = the frame after the jitter operations that precede contrast
//   2. aug_jitter_blur_body        the four ColorJitter operations (per pixel, on the tile + blur halo) -> LDS u8 -> 5 x 9 Gaussian blur from LDS
//   3. aug_resize_post_sharp_body  crop box -> LDS, bilinear resize + posterize of the tile + 1-pixel halo -> LDS u8 -> 3 x 3 sharpness from LDS
// A kernel finds its image b, unpacks the parameters (from its arguments, or from its table entry) and calls the body.  A block serves one image, so in the grouped
// grid (x, frame within its group, group) the entry table[blockIdx.z] is uniform over the block and is read through a uniform address: scalar loads into SGPRs,
// where the single-transform kernels have their kernel arguments.
// No fp32 image goes to memory; the contrast mean is an exact integer sum (no float atomics): a run is bitwise repeatable.  Plain vector stores only.
// Global traffic moves as aligned dwords of the HWC byte stream: a row segment starts at any byte (W * 3 need not be a multiple of 4), so each staged LDS row
// keeps its own 0..3-byte lead and the 0..3 head / tail bytes of a stored segment go out as bytes.
//
// fp contraction is off for the whole file: the contract names separate roundings (r*a + (1-r)*b is two products and a sum), the fused launch must compute bit
// for bit what the same stages compute one launch each, and a grouped launch bit for bit what the single-transform launches compute on each group's slice.
#include "common.h"
#include <stddef.h>
#pragma clang fp contract(off)

#define AUG_NPART 64          // partial sums per image (must match ops.AUG_NPART)
#define AUG_CH 2048           // pixels per staged chunk of the gray reduction
#define AUG_TR 16             // tile rows
#define AUG_TC 128            // tile columns (pixels)
#define AUG_T 256             // threads per block

enum { AUG_BRIGHTNESS = 0, AUG_CONTRAST = 1, AUG_SATURATION = 2, AUG_HUE = 3 };      // torchvision ColorJitter's fn_idx codes

struct AugJitter { int nops; int op0, op1, op2, op3; float f0, f1, f2, f3; };
struct AugBlur { int on; float wx0, wx1, wx2, wx3, wx4, wy0, wy1, wy2, wy3, wy4, wy5, wy6, wy7, wy8; };

// one entry of the grouped form's table (definition in include/svla.h: svla_aug_transform)
struct svla_aug_transform {
    int nops, ops_packed;
    float f[4];
    int nops_before_contrast;
    float wx[5], wy[9];
    int top, left, bh, bw;
    int post_mask, sharpen;
};
#define AUG_FIELD_AT(field, dword) static_assert(offsetof(svla_aug_transform, field) == 4 * (dword), "svla_aug_transform." #field ": not where include/svla.h puts it")
static_assert(sizeof(svla_aug_transform) == 27 * 4, "svla_aug_transform: 27 dwords, no padding");
AUG_FIELD_AT(nops, 0); AUG_FIELD_AT(ops_packed, 1); AUG_FIELD_AT(f, 2); AUG_FIELD_AT(nops_before_contrast, 6); AUG_FIELD_AT(wx, 7); AUG_FIELD_AT(wy, 12);
AUG_FIELD_AT(top, 21); AUG_FIELD_AT(left, 22); AUG_FIELD_AT(bh, 23); AUG_FIELD_AT(bw, 24); AUG_FIELD_AT(post_mask, 25); AUG_FIELD_AT(sharpen, 26);

// operation code k in bits 4k .. 4k + 3 of ops_packed (the host has cleared or refused the bits above 4 * nops)
__host__ __device__ __forceinline__ AugJitter aug_unpack_jitter(int nops, int ops_packed, const float* f) {
    return AugJitter{nops, ops_packed & 15, (ops_packed >> 4) & 15, (ops_packed >> 8) & 15, (ops_packed >> 12) & 15, f[0], f[1], f[2], f[3]};
}

// ---- per-pixel arithmetic ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float aug_blend(float a, float b, float r) {      // trunc(clamp(r a + (1 - r) b, 0, 255))
    float v = r * a + (1.f - r) * b;
    v = fminf(fmaxf(v, 0.f), 255.f);
    return truncf(v);
}
__device__ __forceinline__ float aug_gray(float r, float g, float b) { return truncf(0.2989f * r + 0.587f * g + 0.114f * b); }
__device__ __forceinline__ float aug_clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
__device__ __forceinline__ float aug_round_u8(float v) { return fminf(fmaxf(rintf(v), 0.f), 255.f); }      // round half to even

__device__ __forceinline__ void aug_hue(float& R, float& G, float& B, float hf) {
    const float r = R / 255.f, g = G / 255.f, b = B / 255.f;
    const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
    const bool eq = maxc == minc;
    const float cr = maxc - minc;
    const float s = cr / (eq ? 1.f : maxc);
    const float dv = eq ? 1.f : cr;
    const float rc = (maxc - r) / dv, gc = (maxc - g) / dv, bc = (maxc - b) / dv;
    float h;
    if (maxc == r) h = bc - gc;
    else if (maxc == g) h = 2.f + rc - bc;
    else h = 4.f + gc - rc;
    h = fmodf(h / 6.f + 1.f, 1.f);
    h = fmodf(h + hf, 1.f);
    if (h < 0.f) h += 1.f;                      // (h + f) mod 1 with the sign of the divisor
    const float v = maxc;
    const float h6 = h * 6.f, fi = floorf(h6), f = h6 - fi;
    const int i = ((int)fi) % 6;
    const float p = aug_clamp01(v * (1.f - s)), q = aug_clamp01(v * (1.f - s * f)), t = aug_clamp01(v * (1.f - s * (1.f - f)));
    float o0, o1, o2;
    switch (i) {
        case 0: o0 = v; o1 = t; o2 = p; break;
        case 1: o0 = q; o1 = v; o2 = p; break;
        case 2: o0 = p; o1 = v; o2 = t; break;
        case 3: o0 = p; o1 = q; o2 = v; break;
        case 4: o0 = t; o1 = p; o2 = v; break;
        default: o0 = v; o1 = p; o2 = q; break;
    }
    R = truncf(o0 * 255.999f); G = truncf(o1 * 255.999f); B = truncf(o2 * 255.999f);
}
__device__ __forceinline__ void aug_jitter_one(float& r, float& g, float& b, int op, float f, float mean) {
    if (op == AUG_BRIGHTNESS) { r = aug_blend(r, 0.f, f); g = aug_blend(g, 0.f, f); b = aug_blend(b, 0.f, f); }
    else if (op == AUG_CONTRAST) { r = aug_blend(r, mean, f); g = aug_blend(g, mean, f); b = aug_blend(b, mean, f); }
    else if (op == AUG_SATURATION) { const float y = aug_gray(r, g, b); r = aug_blend(r, y, f); g = aug_blend(g, y, f); b = aug_blend(b, y, f); }
    else aug_hue(r, g, b, f);
}
// the first n operations of the call's order (n = J.nops: all of them; n = the position of contrast: the image whose gray mean contrast needs)
__device__ __forceinline__ void aug_jitter(float& r, float& g, float& b, const AugJitter& J, int n, float mean) {
    if (n > 0) aug_jitter_one(r, g, b, J.op0, J.f0, mean);
    if (n > 1) aug_jitter_one(r, g, b, J.op1, J.f1, mean);
    if (n > 2) aug_jitter_one(r, g, b, J.op2, J.f2, mean);
    if (n > 3) aug_jitter_one(r, g, b, J.op3, J.f3, mean);
}

// ---- dword-wide staging of byte rows ---------------------------------------------------------------------------------------------
// nrows segments of nb bytes (segment r starts at src_of(r), any alignment) -> LDS rows of `pitch` bytes (pitch % 4 == 0, pitch >= nb + 6): byte i of segment r lands
// at lds[r * pitch + (src_of(r) & 3) + i].  Aligned dwords; a dword that is not wholly inside the tensor [tb, te) is assembled from its bytes that are.
template <class F>
__device__ __forceinline__ void aug_stage_rows(unsigned char* lds, int pitch, int nrows, int nb, F src_of, const unsigned char* tb, const unsigned char* te) {
    const int ndw = (nb + 6) / 4;
    for (int i = threadIdx.x; i < nrows * ndw; i += AUG_T) {
        const int r = i / ndw, j = i - r * ndw;
        const unsigned char* g = src_of(r);
        const int lead = (int)((uintptr_t)g & 3);
        if (4 * j >= lead + nb) continue;
        const unsigned char* a = g - lead + 4 * j;
        uint32_t w = 0;
        if (a >= tb && a + 4 <= te) w = *(const uint32_t*)a;
        else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (a + e >= tb && a + e < te) w |= (uint32_t)a[e] << (8 * e);
        }
        *(uint32_t*)(lds + r * pitch + 4 * j) = w;
    }
}
// nrows segments of nb bytes, byte k of segment r = val(r, k), to dst_of(r) (any alignment): aligned dwords inside the segment, its 0..3 head / tail bytes as bytes
template <class F, class V>
__device__ __forceinline__ void aug_store_rows(int nrows, int nb, F dst_of, V val) {
    const int ndw = (nb + 6) / 4;
    for (int i = threadIdx.x; i < nrows * ndw; i += AUG_T) {
        const int r = i / ndw, j = i - r * ndw;
        unsigned char* g = dst_of(r);
        const int lead = (int)((uintptr_t)g & 3);
        if (4 * j >= lead + nb) continue;
        const int lo = 4 * j - lead;
        if (lo >= 0 && lo + 4 <= nb) {
            const uint32_t w = (uint32_t)val(r, lo) | ((uint32_t)val(r, lo + 1) << 8) | ((uint32_t)val(r, lo + 2) << 16) | ((uint32_t)val(r, lo + 3) << 24);
            *(uint32_t*)(g + lo) = w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (lo + e >= 0 && lo + e < nb) g[lo + e] = (unsigned char)val(r, lo + e);
        }
    }
}

// ---- tile geometry and index helpers of the blur and the resize launches ------------------------------------------------------------------
#define AUG_B_ROWS (AUG_TR + 8)
#define AUG_B_PITCH ((AUG_TC + 4) * 3 + 12)
__device__ __forceinline__ int aug_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }      // reflect without edge repeat
#define AUG_CA_ROWS (AUG_TR + 4)
#define AUG_CA_COLS (AUG_TC + 4)
#define AUG_CA_PITCH (AUG_CA_COLS * 3 + 12)
#define AUG_CB_ROWS (AUG_TR + 2)
#define AUG_CB_PITCH ((AUG_TC + 2) * 3 + 2)
// src = (dst + 0.5) in/out - 0.5 clamped at 0; neighbour clamped at the box edge (bilinear, align_corners = False)
__device__ __forceinline__ void aug_src(int d, float scale, int in, int& i0, int& i1, float& l1) {
    float s = ((float)d + 0.5f) * scale - 0.5f;
    s = fmaxf(s, 0.f);
    i0 = min((int)floorf(s), in - 1);
    i1 = min(i0 + 1, in - 1);
    l1 = s - (float)i0;
}

// ---- 1. gray partial sums ----------------------------------------------------------------------------------------------------------
// block (part = blockIdx.x, image b) sums gray(the first `upto` operations of J on x) over its share of image b's pixels as integers
// -> partials[b * AUG_NPART + part]
__device__ __forceinline__ void aug_gray_partials_body(const unsigned char* __restrict__ x, long img_bytes, int npx, int b, const AugJitter& J, int upto,
                                                       unsigned long long* __restrict__ partials, const unsigned char* tb, const unsigned char* te) {
    __shared__ __attribute__((aligned(16))) unsigned char buf[AUG_CH * 3 + 16];
    __shared__ unsigned long long wsum[AUG_T / 64];
    const int part = blockIdx.x;
    const int per = (npx + AUG_NPART - 1) / AUG_NPART;
    const int p0 = part * per, p1 = min(npx, p0 + per);
    const unsigned char* img = x + (size_t)b * img_bytes;
    unsigned long long acc = 0;
    for (int c0 = p0; c0 < p1; c0 += AUG_CH) {
        const int n = min(AUG_CH, p1 - c0);
        const unsigned char* g = img + (size_t)c0 * 3;
        __syncthreads();
        aug_stage_rows(buf, 0, 1, n * 3, [&](int) { return g; }, tb, te);
        __syncthreads();
        const unsigned char* s = buf + ((uintptr_t)g & 3);
        for (int i = threadIdx.x; i < n; i += AUG_T) {
            float r = (float)s[3 * i], gg = (float)s[3 * i + 1], bb = (float)s[3 * i + 2];
            aug_jitter(r, gg, bb, J, upto, 0.f);
            acc += (unsigned long long)(unsigned)aug_gray(r, gg, bb);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
#pragma unroll
        for (int w = 0; w < AUG_T / 64; ++w) t += wsum[w];
        partials[(size_t)b * AUG_NPART + part] = t;
    }
}

// ---- 2. ColorJitter + Gaussian blur ------------------------------------------------------------------------------------------------
// block (tile = blockIdx.x, image b).  The tile's rows y0 - 4 .. y0 + th + 3 (reflected at the image edge) and columns x0 - 2 .. x0 + tw + 1 (clipped; reflected
// when read) are staged, the jitter operations run in place on the staged bytes, the blur reads them.  blur.on == 0: no halo, the jittered tile is stored; a caller
// that always blurs passes blur.on as a literal, so that its halo sizes are compile-time constants.
__device__ __forceinline__ void aug_jitter_blur_body(const unsigned char* __restrict__ x, unsigned char* __restrict__ y, int H, int W, int b, const AugJitter& J,
                                                     const unsigned long long* __restrict__ partials, const AugBlur& blur, const unsigned char* tb,
                                                     const unsigned char* te) {
    __shared__ __attribute__((aligned(16))) unsigned char tile[AUG_B_ROWS * AUG_B_PITCH];
    __shared__ unsigned char leads[AUG_B_ROWS];
    __shared__ float s_mean;
    const int tilesx = (W + AUG_TC - 1) / AUG_TC;
    const int tx = blockIdx.x % tilesx, ty = blockIdx.x / tilesx;
    const int x0 = tx * AUG_TC, y0 = ty * AUG_TR;
    const int tw = min(AUG_TC, W - x0), th = min(AUG_TR, H - y0);
    const int hr = blur.on ? 4 : 0, hc = blur.on ? 2 : 0;
    const int xs = max(x0 - hc, 0), xe = min(x0 + tw + hc, W);
    const int npc = xe - xs, nb = npc * 3, nrows = th + 2 * hr;
    const size_t RB = (size_t)W * 3;
    const unsigned char* img = x + (size_t)b * H * RB;
    auto src_of = [&](int lr) { return img + (size_t)aug_reflect(y0 - hr + lr, H) * RB + (size_t)xs * 3; };
    aug_stage_rows(tile, AUG_B_PITCH, nrows, nb, src_of, tb, te);
    if (threadIdx.x < nrows) leads[threadIdx.x] = (unsigned char)((uintptr_t)src_of(threadIdx.x) & 3);
    const bool has_contrast = (J.nops > 0 && J.op0 == AUG_CONTRAST) || (J.nops > 1 && J.op1 == AUG_CONTRAST) || (J.nops > 2 && J.op2 == AUG_CONTRAST) ||
                              (J.nops > 3 && J.op3 == AUG_CONTRAST);
    if (has_contrast && threadIdx.x < 64) {      // the second pass of the reduction: AUG_NPART integers, summed in any order to the same value
        unsigned long long v = partials[(size_t)b * AUG_NPART + threadIdx.x];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (threadIdx.x == 0) s_mean = (float)((double)v / (double)((long long)H * W));      // the exact mean, rounded once to fp32
    }
    __syncthreads();
    if (J.nops > 0) {
        const float mean = has_contrast ? s_mean : 0.f;
        for (int i = threadIdx.x; i < nrows * npc; i += AUG_T) {
            const int lr = i / npc, c = i - lr * npc;
            unsigned char* p = tile + lr * AUG_B_PITCH + leads[lr] + c * 3;
            float r = (float)p[0], g = (float)p[1], bb = (float)p[2];
            aug_jitter(r, g, bb, J, J.nops, mean);
            p[0] = (unsigned char)r; p[1] = (unsigned char)g; p[2] = (unsigned char)bb;
        }
        __syncthreads();
    }
    unsigned char* yimg = y + (size_t)b * H * RB;
    auto dst_of = [&](int r) { return yimg + (size_t)(y0 + r) * RB + (size_t)x0 * 3; };
    if (!blur.on) {
        aug_store_rows(th, tw * 3, dst_of, [&](int r, int k) { return (unsigned)tile[r * AUG_B_PITCH + leads[r] + k]; });
        return;
    }
    const float wx[5] = {blur.wx0, blur.wx1, blur.wx2, blur.wx3, blur.wx4};
    const float wy[9] = {blur.wy0, blur.wy1, blur.wy2, blur.wy3, blur.wy4, blur.wy5, blur.wy6, blur.wy7, blur.wy8};
    aug_store_rows(th, tw * 3, dst_of, [&](int r, int k) {
        const int px = k / 3, ch = k - 3 * px;
        int off[5];
#pragma unroll
        for (int dx = 0; dx < 5; ++dx) off[dx] = (aug_reflect(x0 + px + dx - 2, W) - xs) * 3 + ch;
        float acc = 0.f;
#pragma unroll
        for (int dy = 0; dy < 9; ++dy) {
            const unsigned char* rp = tile + (r + dy) * AUG_B_PITCH + leads[r + dy];
#pragma unroll
            for (int dx = 0; dx < 5; ++dx) acc = acc + (wy[dy] * wx[dx]) * (float)rp[off[dx]];
        }
        return (unsigned)aug_round_u8(acc);
    });
}

// ---- 3. crop + resize, posterize (x & pmask), sharpness ------------------------------------------------------------------------------
// block (tile = blockIdx.x, image b).  The box is resized to the whole H x W frame (the output never is smaller than the box: the host refuses a box that leaves the
// image, so scale <= 1 and the source rectangle of a tile plus its 1-pixel sharpness halo is at most 2 rows / columns larger than that: 20 x 132 pixels).  Box = the
// whole frame: the resize is the identity, bit for bit.
__device__ __forceinline__ void aug_resize_post_sharp_body(const unsigned char* __restrict__ x, unsigned char* __restrict__ y, int H, int W, int b, int top,
                                                           int left, int bh, int bw, unsigned pmask, int sharpen, const unsigned char* tb,
                                                           const unsigned char* te) {
    __shared__ __attribute__((aligned(16))) unsigned char A[AUG_CA_ROWS * AUG_CA_PITCH];
    __shared__ unsigned char Bt[AUG_CB_ROWS * AUG_CB_PITCH];
    __shared__ unsigned char leads[AUG_CA_ROWS];
    const int tilesx = (W + AUG_TC - 1) / AUG_TC;
    const int tx = blockIdx.x % tilesx, ty = blockIdx.x / tilesx;
    const int x0 = tx * AUG_TC, y0 = ty * AUG_TR;
    const int tw = min(AUG_TC, W - x0), th = min(AUG_TR, H - y0);
    const int hs = sharpen ? 1 : 0;
    const int ya = max(y0 - hs, 0), yb = min(y0 + th + hs, H), xa = max(x0 - hs, 0), xb = min(x0 + tw + hs, W);
    const float sy = (float)bh / (float)H, sx = (float)bw / (float)W;
    int sya, syb, sxa, sxb, t0, t1;
    float tl;
    aug_src(ya, sy, bh, sya, t1, tl);
    aug_src(yb - 1, sy, bh, t0, syb, tl);
    aug_src(xa, sx, bw, sxa, t1, tl);
    aug_src(xb - 1, sx, bw, t0, sxb, tl);
    const int nrA = min(syb - sya + 1, AUG_CA_ROWS), ncA = min(sxb - sxa + 1, AUG_CA_COLS);
    const size_t RB = (size_t)W * 3;
    const unsigned char* img = x + (size_t)b * H * RB;
    auto src_of = [&](int lr) { return img + (size_t)(top + sya + lr) * RB + (size_t)(left + sxa) * 3; };
    aug_stage_rows(A, AUG_CA_PITCH, nrA, ncA * 3, src_of, tb, te);
    if (threadIdx.x < nrA) leads[threadIdx.x] = (unsigned char)((uintptr_t)src_of(threadIdx.x) & 3);
    __syncthreads();
    const int nby = yb - ya, nbx = xb - xa;
    for (int i = threadIdx.x; i < nby * nbx; i += AUG_T) {
        const int ry = i / nbx, rx = i - ry * nbx;
        int y0i, y1i, x0i, x1i;
        float ly, lx;
        aug_src(ya + ry, sy, bh, y0i, y1i, ly);
        aug_src(xa + rx, sx, bw, x0i, x1i, lx);
        y0i = min(y0i - sya, nrA - 1); y1i = min(y1i - sya, nrA - 1); x0i = min(x0i - sxa, ncA - 1); x1i = min(x1i - sxa, ncA - 1);
        const unsigned char* r0 = A + y0i * AUG_CA_PITCH + leads[y0i];
        const unsigned char* r1 = A + y1i * AUG_CA_PITCH + leads[y1i];
        const float ly0 = 1.f - ly, lx0 = 1.f - lx;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float a = (float)r0[x0i * 3 + ch], bq = (float)r0[x1i * 3 + ch], c = (float)r1[x0i * 3 + ch], d = (float)r1[x1i * 3 + ch];
            const float v = ly0 * (lx0 * a + lx * bq) + ly * (lx0 * c + lx * d);
            Bt[ry * AUG_CB_PITCH + rx * 3 + ch] = (unsigned char)((unsigned)aug_round_u8(v) & pmask);
        }
    }
    __syncthreads();
    unsigned char* yimg = y + (size_t)b * H * RB;
    auto dst_of = [&](int r) { return yimg + (size_t)(y0 + r) * RB + (size_t)x0 * 3; };
    const float w1 = 1.f / 13.f, w5 = 5.f / 13.f;
    aug_store_rows(th, tw * 3, dst_of, [&](int r, int k) {
        const int px = k / 3, ch = k - 3 * px;
        const int oy = y0 + r, ox = x0 + px;
        const unsigned char* c = Bt + (oy - ya) * AUG_CB_PITCH + (ox - xa) * 3 + ch;
        const float v = (float)c[0];
        if (!sharpen || oy < 1 || oy > H - 2 || ox < 1 || ox > W - 2) return (unsigned)v;      // border pixels keep x
        float acc = 0.f;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) acc = acc + ((dy == 0 && dx == 0) ? w5 : w1) * (float)c[dy * AUG_CB_PITCH + dx * 3];
        return (unsigned)aug_blend(v, aug_round_u8(acc), 2.f);
    });
}

// ---- the six kernels: find the image, unpack its parameters, call the body -----------------------------------------------------------------
// single-transform: grid (AUG_NPART or tiles, B), parameters by value.  The gray reduction applies all the operations it was given.
__global__ void __launch_bounds__(AUG_T) aug_gray_partials_kernel(const unsigned char* __restrict__ x, long img_bytes, int npx, AugJitter J, int upto,
                                                                  unsigned long long* __restrict__ partials, const unsigned char* tb, const unsigned char* te) {
    aug_gray_partials_body(x, img_bytes, npx, blockIdx.y, J, upto, partials, tb, te);
}
__global__ void __launch_bounds__(AUG_T) aug_jitter_blur_kernel(const unsigned char* __restrict__ x, unsigned char* __restrict__ y, int H, int W, AugJitter J,
                                                                const unsigned long long* __restrict__ partials, AugBlur blur, const unsigned char* tb,
                                                                const unsigned char* te) {
    aug_jitter_blur_body(x, y, H, W, blockIdx.y, J, partials, blur, tb, te);
}
__global__ void __launch_bounds__(AUG_T) aug_resize_post_sharp_kernel(const unsigned char* __restrict__ x, unsigned char* __restrict__ y, int H, int W, int top,
                                                                      int left, int bh, int bw, int posterize, int sharpen, const unsigned char* tb,
                                                                      const unsigned char* te) {
    aug_resize_post_sharp_body(x, y, H, W, blockIdx.y, top, left, bh, bw, posterize ? 0xFEu : 0xFFu, sharpen, tb, te);
}

// grouped: grid (AUG_NPART or tiles, group_len, G), parameters from table[blockIdx.z].  A group whose order has no contrast (nops_before_contrast < 0) needs no
// mean: its blocks of the gray reduction leave their partials unwritten.  The blur is always on (the list applies GaussianBlur unconditionally).
__global__ void __launch_bounds__(AUG_T) aug_gray_partials_grouped_kernel(const unsigned char* __restrict__ x, long img_bytes, int npx,
                                                                          const svla_aug_transform* __restrict__ table, unsigned long long* __restrict__ partials,
                                                                          const unsigned char* tb, const unsigned char* te) {
    const svla_aug_transform& t = table[blockIdx.z];
    if (t.nops_before_contrast < 0) return;
    aug_gray_partials_body(x, img_bytes, npx, blockIdx.z * gridDim.y + blockIdx.y, aug_unpack_jitter(t.nops, t.ops_packed, t.f), t.nops_before_contrast, partials, tb,
                           te);
}
__global__ void __launch_bounds__(AUG_T) aug_jitter_blur_grouped_kernel(const unsigned char* __restrict__ x, unsigned char* __restrict__ y, int H, int W,
                                                                        const svla_aug_transform* __restrict__ table,
                                                                        const unsigned long long* __restrict__ partials, const unsigned char* tb,
                                                                        const unsigned char* te) {
    const svla_aug_transform& t = table[blockIdx.z];
    aug_jitter_blur_body(x, y, H, W, blockIdx.z * gridDim.y + blockIdx.y, aug_unpack_jitter(t.nops, t.ops_packed, t.f), partials,
                         AugBlur{1, t.wx[0], t.wx[1], t.wx[2], t.wx[3], t.wx[4], t.wy[0], t.wy[1], t.wy[2], t.wy[3], t.wy[4], t.wy[5], t.wy[6], t.wy[7], t.wy[8]}, tb,
                         te);
}
__global__ void __launch_bounds__(AUG_T) aug_resize_post_sharp_grouped_kernel(const unsigned char* __restrict__ x, unsigned char* __restrict__ y, int H, int W,
                                                                              const svla_aug_transform* __restrict__ table, const unsigned char* tb,
                                                                              const unsigned char* te) {
    const svla_aug_transform& t = table[blockIdx.z];
    aug_resize_post_sharp_body(x, y, H, W, blockIdx.z * gridDim.y + blockIdx.y, t.top, t.left, t.bh, t.bw, (unsigned)t.post_mask, t.sharpen, tb, te);
}

// ---- host checks -----------------------------------------------------------------------------------------------------------------------
// every entry validates everything (the grouped form: the whole HOST table) before anything is enqueued: a refused call launches nothing and copies nothing
static inline int aug_tiles(int H, int W) { return ((H + AUG_TR - 1) / AUG_TR) * ((W + AUG_TC - 1) / AUG_TC); }
static inline bool aug_frame_ok(int H, int W) {      // the reflect padding needs H >= 5, W >= 3; image bytes and tile count fit an int
    return H >= 5 && W >= 3 && (long long)H * W * 3 < (1ll << 31) && ((long long)(H + AUG_TR - 1) / AUG_TR) * ((W + AUG_TC - 1) / AUG_TC) < (1ll << 31);
}
// at most four known operation codes; contrast_at = the position of the first contrast, -1 without one
static inline bool aug_ops_ok(int nops, int ops_packed, int& contrast_at) {
    if (nops < 0 || nops > 4) return false;
    contrast_at = -1;
    for (int k = 0; k < nops; ++k) {
        const int op = (ops_packed >> (4 * k)) & 15;
        if (op > AUG_HUE) return false;
        if (op == AUG_CONTRAST && contrast_at < 0) contrast_at = k;
    }
    return true;
}
static inline bool aug_box_ok(int H, int W, int top, int left, int bh, int bw) {      // the crop box lies inside the image
    return top >= 0 && left >= 0 && bh >= 1 && bw >= 1 && (long long)top + bh <= H && (long long)left + bw <= W;
}
static inline bool aug_single_ok(int B, int H, int W) { return B > 0 && B <= 65535 && aug_frame_ok(H, W); }
// the single-transform form's J: the bits of ops_packed above 4 * nops are not the caller's to set and do not reach the kernel
static inline bool aug_single_jitter(int nops, int ops_packed, const float* f, AugJitter& J, int& contrast_at) {
    if (!aug_ops_ok(nops, ops_packed, contrast_at)) return false;
    J = aug_unpack_jitter(nops, ops_packed & ((1 << (4 * nops)) - 1), f);
    return true;
}
static bool aug_grouped_ok(int N, int H, int W, int group_len, const svla_aug_transform* th, const void* td) {
    if (!th || !td || N <= 0 || group_len <= 0 || group_len > 65535 || N % group_len != 0 || N / group_len > 65535 || !aug_frame_ok(H, W)) return false;
    for (int g = 0; g < N / group_len; ++g) {
        const svla_aug_transform& t = th[g];
        int contrast_at;
        if (!aug_ops_ok(t.nops, t.ops_packed, contrast_at) || (t.ops_packed >> (4 * t.nops)) != 0 || t.nops_before_contrast != contrast_at) return false;
        if (!aug_box_ok(H, W, t.top, t.left, t.bh, t.bw)) return false;
        if (t.post_mask != 0xFF && t.post_mask != 0xFE && t.post_mask != 0xFC && t.post_mask != 0xF8 && t.post_mask != 0xF0) return false;
        if (t.sharpen != 0 && t.sharpen != 1) return false;
    }
    return true;
}
// the table goes to the device scratch on the stream, in front of the launch that reads it (a pageable source is staged before the copy call returns)
static int aug_table_upload(const svla_aug_transform* th, svla_aug_transform* td, int G, hipStream_t s) {
    return svla_memcpy_async(td, th, (size_t)G * sizeof(svla_aug_transform), hipMemcpyHostToDevice, s);
}

// ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
extern "C" int svla_aug_gray_partials(const unsigned char* x, int B, int H, int W, int nops, int ops_packed, float f0, float f1, float f2, float f3,
                                      unsigned long long* partials, void* stream) {
    if (!x || !partials || !aug_single_ok(B, H, W)) return SVLA_EINVAL;
    AugJitter J;
    int contrast_at;
    const float f[4] = {f0, f1, f2, f3};
    if (!aug_single_jitter(nops, ops_packed, f, J, contrast_at)) return SVLA_EINVAL;
    const long img_bytes = (long)H * W * 3;
    return svla_launch<aug_gray_partials_kernel>(dim3(AUG_NPART, B), dim3(AUG_T), 0, (hipStream_t)stream, x, img_bytes, H * W, J, nops, partials, x,
                       x + (size_t)B * img_bytes);
}

extern "C" int svla_aug_jitter_blur_u8(const unsigned char* x, unsigned char* y, int B, int H, int W, int nops, int ops_packed, float f0, float f1, float f2,
                                       float f3, const unsigned long long* partials, const float* wx5, const float* wy9, void* stream) {
    if (!x || !y || x == y || !aug_single_ok(B, H, W) || ((wx5 == nullptr) != (wy9 == nullptr))) return SVLA_EINVAL;
    AugJitter J;
    int contrast_at;
    const float f[4] = {f0, f1, f2, f3};
    if (!aug_single_jitter(nops, ops_packed, f, J, contrast_at)) return SVLA_EINVAL;
    if (contrast_at >= 0 && !partials) return SVLA_EINVAL;
    AugBlur bl{};
    if (wx5) bl = AugBlur{1, wx5[0], wx5[1], wx5[2], wx5[3], wx5[4], wy9[0], wy9[1], wy9[2], wy9[3], wy9[4], wy9[5], wy9[6], wy9[7], wy9[8]};
    return svla_launch<aug_jitter_blur_kernel>(dim3(aug_tiles(H, W), B), dim3(AUG_T), 0, (hipStream_t)stream, x, y, H, W, J, partials, bl, x,
                       x + (size_t)B * H * W * 3);
}

extern "C" int svla_aug_resize_post_sharp_u8(const unsigned char* x, unsigned char* y, int B, int H, int W, int top, int left, int bh, int bw, int posterize,
                                             int sharpen, void* stream) {
    if (!x || !y || x == y || !aug_single_ok(B, H, W) || !aug_box_ok(H, W, top, left, bh, bw)) return SVLA_EINVAL;
    return svla_launch<aug_resize_post_sharp_kernel>(dim3(aug_tiles(H, W), B), dim3(AUG_T), 0, (hipStream_t)stream, x, y, H, W, top, left, bh, bw,
                       posterize ? 1 : 0, sharpen ? 1 : 0, x, x + (size_t)B * H * W * 3);
}

extern "C" int svla_aug_gray_partials_grouped(const unsigned char* x, int N, int H, int W, int group_len, const svla_aug_transform* table_host,
                                              svla_aug_transform* table_dev, unsigned long long* partials, void* stream) {
    if (!x || !partials || !aug_grouped_ok(N, H, W, group_len, table_host, table_dev)) return SVLA_EINVAL;
    const int G = N / group_len;
    if (const int rc = aug_table_upload(table_host, table_dev, G, (hipStream_t)stream)) return rc;
    const long img_bytes = (long)H * W * 3;
    return svla_launch<aug_gray_partials_grouped_kernel>(dim3(AUG_NPART, group_len, G), dim3(AUG_T), 0, (hipStream_t)stream, x, img_bytes, H * W, table_dev, partials,
                       x, x + (size_t)N * img_bytes);
}

extern "C" int svla_aug_jitter_blur_grouped_u8(const unsigned char* x, unsigned char* y, int N, int H, int W, int group_len, const svla_aug_transform* table_host,
                                               svla_aug_transform* table_dev, const unsigned long long* partials, void* stream) {
    if (!x || !y || x == y || !aug_grouped_ok(N, H, W, group_len, table_host, table_dev)) return SVLA_EINVAL;
    const int G = N / group_len;
    for (int g = 0; g < G; ++g)
        if (table_host[g].nops_before_contrast >= 0 && !partials) return SVLA_EINVAL;
    if (const int rc = aug_table_upload(table_host, table_dev, G, (hipStream_t)stream)) return rc;
    return svla_launch<aug_jitter_blur_grouped_kernel>(dim3(aug_tiles(H, W), group_len, G), dim3(AUG_T), 0, (hipStream_t)stream, x, y, H, W, table_dev, partials, x,
                       x + (size_t)N * H * W * 3);
}

extern "C" int svla_aug_resize_post_sharp_grouped_u8(const unsigned char* x, unsigned char* y, int N, int H, int W, int group_len,
                                                     const svla_aug_transform* table_host, svla_aug_transform* table_dev, void* stream) {
    if (!x || !y || x == y || !aug_grouped_ok(N, H, W, group_len, table_host, table_dev)) return SVLA_EINVAL;
    const int G = N / group_len;
    if (const int rc = aug_table_upload(table_host, table_dev, G, (hipStream_t)stream)) return rc;
    return svla_launch<aug_resize_post_sharp_grouped_kernel>(dim3(aug_tiles(H, W), group_len, G), dim3(AUG_T), 0, (hipStream_t)stream, x, y, H, W, table_dev, x,
                       x + (size_t)N * H * W * 3);
}
