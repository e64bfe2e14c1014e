// Sampled frame augmentation of the camera preprocessors (architecture/allenact_preprocessors/dino_preprocessors.py:224-239 applies the transform that
// utils/transformation_util.py:54-119 samples from the v2 list :12-28) as u8 -> u8 kernels in front of svla_normalize_u8_f32 / svla_patchify_u8_bf16.
//
// Arithmetic contract (DESIGN.md "Sampled frame augmentation"): every stage takes and returns u8, every intermediate is rounded to u8 where the torchvision
// op list rounds it.  Three launches per camera per call:
//   1. aug_gray_partials_kernel   integer partial sums of gray(x) per image, x = the frame after the jitter operations that precede contrast
//   2. aug_jitter_blur_kernel     the four ColorJitter operations (per pixel, on the tile + blur halo) -> LDS u8 -> 5 x 9 Gaussian blur from LDS
//   3. aug_resize_post_sharp_kernel  crop box -> LDS, bilinear resize + posterize of the tile + 1-pixel halo -> LDS u8 -> 3 x 3 sharpness from LDS
// No fp32 image goes to memory; the contrast mean is an exact integer sum (no float atomics): a run is bitwise repeatable.
// Global traffic moves as aligned dwords of the HWC byte stream: a row segment starts at any byte (W * 3 need not be a multiple of 4), so each staged LDS row
// keeps its own 0..3-byte lead and the 0..3 head / tail bytes of a stored segment go out as bytes.
//
// fp contraction is off for the whole file (augment_common.h): the contract names separate roundings (r*a + (1-r)*b is two products and a sum), and the fused launch must
// compute bit for bit what the same stages compute one launch each.
#include "augment_common.h"

// ---- 1. gray partial sums ----------------------------------------------------------------------------------------------------------
// grid (AUG_NPART, B): block (p, b) sums gray(jitter_upto(x)) over its share of image b's pixels as integers -> partials[b * AUG_NPART + p]
__global__ void __launch_bounds__(AUG_T) aug_gray_partials_kernel(const unsigned char* __restrict__ x, long img_bytes, int npx, AugJitter J, int upto,
                                                                  unsigned long long* __restrict__ partials, const unsigned char* tb, const unsigned char* te) {
    __shared__ __attribute__((aligned(16))) unsigned char buf[AUG_CH * 3 + 16];
    __shared__ unsigned long long wsum[AUG_T / 64];
    const int b = blockIdx.y, part = blockIdx.x;
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
// grid (tiles, B).  The tile's rows y0 - 4 .. y0 + th + 3 (reflected at the image edge) and columns x0 - 2 .. x0 + tw + 1 (clipped; reflected when read) are staged,
// the jitter operations run in place on the staged bytes, the blur reads them.  blur.on == 0: no halo, the jittered tile is stored.
__global__ void __launch_bounds__(AUG_T) aug_jitter_blur_kernel(const unsigned char* __restrict__ x, unsigned char* __restrict__ y, int H, int W, AugJitter J,
                                                                const unsigned long long* __restrict__ partials, AugBlur blur, const unsigned char* tb,
                                                                const unsigned char* te) {
    __shared__ __attribute__((aligned(16))) unsigned char tile[AUG_B_ROWS * AUG_B_PITCH];
    __shared__ unsigned char leads[AUG_B_ROWS];
    __shared__ float s_mean;
    const int tilesx = (W + AUG_TC - 1) / AUG_TC;
    const int tx = blockIdx.x % tilesx, ty = blockIdx.x / tilesx, b = blockIdx.y;
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

// ---- 3. crop + resize, posterize, sharpness ------------------------------------------------------------------------------------------
// grid (tiles, B).  The box is resized to the whole H x W frame (the output never is smaller than the box: scale <= 1, so the source rectangle of a tile plus its
// 1-pixel sharpness halo is at most 2 rows / columns larger than that).  Box = the whole frame: the resize is the identity, bit for bit.
__global__ void __launch_bounds__(AUG_T) aug_resize_post_sharp_kernel(const unsigned char* __restrict__ x, unsigned char* __restrict__ y, int H, int W, int top,
                                                                      int left, int bh, int bw, int posterize, int sharpen, const unsigned char* tb,
                                                                      const unsigned char* te) {
    __shared__ __attribute__((aligned(16))) unsigned char A[AUG_CA_ROWS * AUG_CA_PITCH];
    __shared__ unsigned char Bt[AUG_CB_ROWS * AUG_CB_PITCH];
    __shared__ unsigned char leads[AUG_CA_ROWS];
    const int tilesx = (W + AUG_TC - 1) / AUG_TC;
    const int tx = blockIdx.x % tilesx, ty = blockIdx.x / tilesx, b = blockIdx.y;
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
    const unsigned pmask = posterize ? 0xFEu : 0xFFu;
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

// ---- C ABI ---------------------------------------------------------------------------------------------------------------------------
static bool aug_shape_ok(int B, int H, int W) {
    return B > 0 && B <= 65535 && H >= 5 && W >= 3 && (long long)H * W * 3 < (1ll << 31) && ((long long)(H + AUG_TR - 1) / AUG_TR) * ((W + AUG_TC - 1) / AUG_TC) < (1ll << 31);
}
static bool aug_jitter_ok(int nops, int ops_packed, AugJitter& J, const float* f, int& contrast_at) {
    if (nops < 0 || nops > 4) return false;
    int op[4] = {0, 0, 0, 0};
    contrast_at = -1;
    for (int k = 0; k < nops; ++k) {
        op[k] = (ops_packed >> (4 * k)) & 15;
        if (op[k] > AUG_HUE) return false;
        if (op[k] == AUG_CONTRAST && contrast_at < 0) contrast_at = k;
    }
    J = AugJitter{nops, op[0], op[1], op[2], op[3], f[0], f[1], f[2], f[3]};
    return true;
}

extern "C" int svla_aug_gray_partials(const unsigned char* x, int B, int H, int W, int nops, int ops_packed, float f0, float f1, float f2, float f3,
                                      unsigned long long* partials, void* stream) {
    if (!x || !partials || !aug_shape_ok(B, H, W)) return SVLA_EINVAL;
    AugJitter J;
    int contrast_at;
    const float f[4] = {f0, f1, f2, f3};
    if (!aug_jitter_ok(nops, ops_packed, J, f, contrast_at)) return SVLA_EINVAL;
    const long img_bytes = (long)H * W * 3;
    hipLaunchKernelGGL(aug_gray_partials_kernel, dim3(AUG_NPART, B), dim3(AUG_T), 0, (hipStream_t)stream, x, img_bytes, H * W, J, nops, partials, x,
                       x + (size_t)B * img_bytes);
    return svla_launch_status();
}

extern "C" int svla_aug_jitter_blur_u8(const unsigned char* x, unsigned char* y, int B, int H, int W, int nops, int ops_packed, float f0, float f1, float f2,
                                       float f3, const unsigned long long* partials, const float* wx5, const float* wy9, void* stream) {
    if (!x || !y || x == y || !aug_shape_ok(B, H, W) || ((wx5 == nullptr) != (wy9 == nullptr))) return SVLA_EINVAL;
    AugJitter J;
    int contrast_at;
    const float f[4] = {f0, f1, f2, f3};
    if (!aug_jitter_ok(nops, ops_packed, J, f, contrast_at)) return SVLA_EINVAL;
    if (contrast_at >= 0 && !partials) return SVLA_EINVAL;
    AugBlur bl{};
    if (wx5) bl = AugBlur{1, wx5[0], wx5[1], wx5[2], wx5[3], wx5[4], wy9[0], wy9[1], wy9[2], wy9[3], wy9[4], wy9[5], wy9[6], wy9[7], wy9[8]};
    const int tiles = ((H + AUG_TR - 1) / AUG_TR) * ((W + AUG_TC - 1) / AUG_TC);
    hipLaunchKernelGGL(aug_jitter_blur_kernel, dim3(tiles, B), dim3(AUG_T), 0, (hipStream_t)stream, x, y, H, W, J, partials, bl, x, x + (size_t)B * H * W * 3);
    return svla_launch_status();
}

extern "C" int svla_aug_resize_post_sharp_u8(const unsigned char* x, unsigned char* y, int B, int H, int W, int top, int left, int bh, int bw, int posterize,
                                             int sharpen, void* stream) {
    if (!x || !y || x == y || !aug_shape_ok(B, H, W)) return SVLA_EINVAL;
    if (top < 0 || left < 0 || bh < 1 || bw < 1 || (long long)top + bh > H || (long long)left + bw > W) return SVLA_EINVAL;      // crop box outside the image
    const int tiles = ((H + AUG_TR - 1) / AUG_TR) * ((W + AUG_TC - 1) / AUG_TC);
    hipLaunchKernelGGL(aug_resize_post_sharp_kernel, dim3(tiles, B), dim3(AUG_T), 0, (hipStream_t)stream, x, y, H, W, top, left, bh, bw, posterize ? 1 : 0,
                       sharpen ? 1 : 0, x, x + (size_t)B * H * W * 3);
    return svla_launch_status();
}
