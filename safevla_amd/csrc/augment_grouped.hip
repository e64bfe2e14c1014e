// Per-trajectory random frame augmentation: the three launches of augment.hip with one transform per GROUP of frames instead of one for the whole batch.  The
// imitation-learning Preprocessor (architecture/models/transformer_models/preprocessors.py:86-118) applies the full random v2 list
// (utils/transformation_util.py:12-28) once per trajectory and camera to that trajectory's [T, 3, H, W] frames, every call with newly drawn parameters; a batch
// [B, T, H, W, 3] therefore carries B transforms.  Image n of the [N, H, W, 3] batch uses entry n / group_len of a [G] table of svla_aug_transform in device memory.
//
// Grid (x, frame within its group, group): a block serves one image, so its table entry is uniform over the block and is read through a uniform address (scalar
// loads into SGPRs, as kernel arguments are).  The kernels are those of augment.hip, statement for statement, on the helpers of augment_common.h; only where the
// parameters come from differs (augment.hip stays a translation unit of its own so that its device code does not move).  Posterize is x & post_mask (0xFF: off; 0xFE .. 0xF0: 7 .. 4 bits kept).  Plain vector stores only, no atomics; the integer gray partials stay exact.
//
// fp contraction is off (augment_common.h): a grouped launch computes bit for bit what the single-transform launches compute on each group's slice.
#include "augment_common.h"

// one entry of the table (definition in include/svla.h: svla_aug_transform)
struct svla_aug_transform {
    int nops, ops_packed;
    float f[4];
    int nops_before_contrast;
    float wx[5], wy[9];
    int top, left, bh, bw;
    int post_mask, sharpen;
};
#include <stddef.h>
#define AUG_FIELD_AT(field, dword) static_assert(offsetof(svla_aug_transform, field) == 4 * (dword), "svla_aug_transform." #field ": not where include/svla.h puts it")
static_assert(sizeof(svla_aug_transform) == 27 * 4, "svla_aug_transform: 27 dwords, no padding");
AUG_FIELD_AT(nops, 0); AUG_FIELD_AT(ops_packed, 1); AUG_FIELD_AT(f, 2); AUG_FIELD_AT(nops_before_contrast, 6); AUG_FIELD_AT(wx, 7); AUG_FIELD_AT(wy, 12);
AUG_FIELD_AT(top, 21); AUG_FIELD_AT(left, 22); AUG_FIELD_AT(bh, 23); AUG_FIELD_AT(bw, 24); AUG_FIELD_AT(post_mask, 25); AUG_FIELD_AT(sharpen, 26);

__device__ __forceinline__ AugJitter aug_table_jitter(const svla_aug_transform& t) {
    return AugJitter{t.nops, t.ops_packed & 15, (t.ops_packed >> 4) & 15, (t.ops_packed >> 8) & 15, (t.ops_packed >> 12) & 15, t.f[0], t.f[1], t.f[2], t.f[3]};
}

// ---- 1. gray partial sums ----------------------------------------------------------------------------------------------------------
// grid (AUG_NPART, group_len, G).  A group whose order has no contrast (nops_before_contrast < 0) needs no mean: its blocks leave their partials unwritten.
__global__ void __launch_bounds__(AUG_T) aug_gray_partials_grouped_kernel(const unsigned char* __restrict__ x, long img_bytes, int npx,
                                                                          const svla_aug_transform* __restrict__ table, unsigned long long* __restrict__ partials,
                                                                          const unsigned char* tb, const unsigned char* te) {
    __shared__ __attribute__((aligned(16))) unsigned char buf[AUG_CH * 3 + 16];
    __shared__ unsigned long long wsum[AUG_T / 64];
    const svla_aug_transform& t = table[blockIdx.z];
    const int upto = t.nops_before_contrast;
    if (upto < 0) return;
    const AugJitter J = aug_table_jitter(t);
    const int b = blockIdx.z * gridDim.y + blockIdx.y, part = blockIdx.x;
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
        unsigned long long total = 0;
#pragma unroll
        for (int w = 0; w < AUG_T / 64; ++w) total += wsum[w];
        partials[(size_t)b * AUG_NPART + part] = total;
    }
}

// ---- 2. ColorJitter + Gaussian blur (always on: the list applies GaussianBlur unconditionally) -----------------------------------------
// grid (tiles, group_len, G)
__global__ void __launch_bounds__(AUG_T) aug_jitter_blur_grouped_kernel(const unsigned char* __restrict__ x, unsigned char* __restrict__ y, int H, int W,
                                                                        const svla_aug_transform* __restrict__ table,
                                                                        const unsigned long long* __restrict__ partials, const unsigned char* tb,
                                                                        const unsigned char* te) {
    __shared__ __attribute__((aligned(16))) unsigned char tile[AUG_B_ROWS * AUG_B_PITCH];
    __shared__ unsigned char leads[AUG_B_ROWS];
    __shared__ float s_mean;
    const int tilesx = (W + AUG_TC - 1) / AUG_TC;
    const int tx = blockIdx.x % tilesx, ty = blockIdx.x / tilesx, b = blockIdx.z * gridDim.y + blockIdx.y;
    const svla_aug_transform& t = table[blockIdx.z];
    const AugJitter J = aug_table_jitter(t);
    const int x0 = tx * AUG_TC, y0 = ty * AUG_TR;
    const int tw = min(AUG_TC, W - x0), th = min(AUG_TR, H - y0);
    const int hr = 4, hc = 2;
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
    const float wx[5] = {t.wx[0], t.wx[1], t.wx[2], t.wx[3], t.wx[4]};
    const float wy[9] = {t.wy[0], t.wy[1], t.wy[2], t.wy[3], t.wy[4], t.wy[5], t.wy[6], t.wy[7], t.wy[8]};
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
// grid (tiles, group_len, G).  The LDS bound of augment.hip holds for every entry: the output never is smaller than the box (the host refuses a box that leaves the
// image), so the source rectangle of a tile plus its 1-pixel sharpness halo is at most 20 x 132 pixels.
__global__ void __launch_bounds__(AUG_T) aug_resize_post_sharp_grouped_kernel(const unsigned char* __restrict__ x, unsigned char* __restrict__ y, int H, int W,
                                                                              const svla_aug_transform* __restrict__ table, const unsigned char* tb,
                                                                              const unsigned char* te) {
    __shared__ __attribute__((aligned(16))) unsigned char A[AUG_CA_ROWS * AUG_CA_PITCH];
    __shared__ unsigned char Bt[AUG_CB_ROWS * AUG_CB_PITCH];
    __shared__ unsigned char leads[AUG_CA_ROWS];
    const int tilesx = (W + AUG_TC - 1) / AUG_TC;
    const int tx = blockIdx.x % tilesx, ty = blockIdx.x / tilesx, b = blockIdx.z * gridDim.y + blockIdx.y;
    const svla_aug_transform& t = table[blockIdx.z];
    const int top = t.top, left = t.left, bh = t.bh, bw = t.bw, sharpen = t.sharpen;
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
    const unsigned pmask = (unsigned)t.post_mask;
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
// every entry validates the whole HOST table before anything is enqueued: a refused call launches nothing and copies nothing
static bool aug_grouped_ok(int N, int H, int W, int group_len, const svla_aug_transform* th, const void* td) {
    if (!th || !td || N <= 0 || group_len <= 0 || group_len > 65535 || N % group_len != 0 || N / group_len > 65535 || H < 5 || W < 3) return false;
    if ((long long)H * W * 3 >= (1ll << 31) || ((long long)(H + AUG_TR - 1) / AUG_TR) * ((W + AUG_TC - 1) / AUG_TC) >= (1ll << 31)) return false;
    for (int g = 0; g < N / group_len; ++g) {
        const svla_aug_transform& t = th[g];
        if (t.nops < 0 || t.nops > 4 || (t.ops_packed >> (4 * t.nops)) != 0) return false;
        int contrast_at = -1;
        for (int k = 0; k < t.nops; ++k) {
            const int op = (t.ops_packed >> (4 * k)) & 15;
            if (op > AUG_HUE) return false;
            if (op == AUG_CONTRAST && contrast_at < 0) contrast_at = k;
        }
        if (t.nops_before_contrast != contrast_at) return false;
        if (t.top < 0 || t.left < 0 || t.bh < 1 || t.bw < 1 || (long long)t.top + t.bh > H || (long long)t.left + t.bw > W) return false;      // box outside the image
        if (t.post_mask != 0xFF && t.post_mask != 0xFE && t.post_mask != 0xFC && t.post_mask != 0xF8 && t.post_mask != 0xF0) return false;
        if (t.sharpen != 0 && t.sharpen != 1) return false;
    }
    return true;
}
// the table goes to the device scratch on the stream, in front of the launch that reads it (a pageable source is staged before hipMemcpyAsync returns)
static int aug_table_upload(const svla_aug_transform* th, svla_aug_transform* td, int G, hipStream_t s) {
    HIP_CHECK_RET(hipMemcpyAsync(td, th, (size_t)G * sizeof(svla_aug_transform), hipMemcpyHostToDevice, s));
    return SVLA_OK;
}

extern "C" int svla_aug_gray_partials_grouped(const unsigned char* x, int N, int H, int W, int group_len, const svla_aug_transform* table_host,
                                              svla_aug_transform* table_dev, unsigned long long* partials, void* stream) {
    if (!x || !partials || !aug_grouped_ok(N, H, W, group_len, table_host, table_dev)) return SVLA_EINVAL;
    const int G = N / group_len;
    if (const int rc = aug_table_upload(table_host, table_dev, G, (hipStream_t)stream)) return rc;
    const long img_bytes = (long)H * W * 3;
    hipLaunchKernelGGL(aug_gray_partials_grouped_kernel, dim3(AUG_NPART, group_len, G), dim3(AUG_T), 0, (hipStream_t)stream, x, img_bytes, H * W, table_dev, partials,
                       x, x + (size_t)N * img_bytes);
    return svla_launch_status();
}

extern "C" int svla_aug_jitter_blur_grouped_u8(const unsigned char* x, unsigned char* y, int N, int H, int W, int group_len, const svla_aug_transform* table_host,
                                               svla_aug_transform* table_dev, const unsigned long long* partials, void* stream) {
    if (!x || !y || x == y || !aug_grouped_ok(N, H, W, group_len, table_host, table_dev)) return SVLA_EINVAL;
    const int G = N / group_len;
    for (int g = 0; g < G; ++g)
        if (table_host[g].nops_before_contrast >= 0 && !partials) return SVLA_EINVAL;
    if (const int rc = aug_table_upload(table_host, table_dev, G, (hipStream_t)stream)) return rc;
    const int tiles = ((H + AUG_TR - 1) / AUG_TR) * ((W + AUG_TC - 1) / AUG_TC);
    hipLaunchKernelGGL(aug_jitter_blur_grouped_kernel, dim3(tiles, group_len, G), dim3(AUG_T), 0, (hipStream_t)stream, x, y, H, W, table_dev, partials, x,
                       x + (size_t)N * H * W * 3);
    return svla_launch_status();
}

extern "C" int svla_aug_resize_post_sharp_grouped_u8(const unsigned char* x, unsigned char* y, int N, int H, int W, int group_len,
                                                     const svla_aug_transform* table_host, svla_aug_transform* table_dev, void* stream) {
    if (!x || !y || x == y || !aug_grouped_ok(N, H, W, group_len, table_host, table_dev)) return SVLA_EINVAL;
    const int G = N / group_len;
    if (const int rc = aug_table_upload(table_host, table_dev, G, (hipStream_t)stream)) return rc;
    const int tiles = ((H + AUG_TR - 1) / AUG_TR) * ((W + AUG_TC - 1) / AUG_TC);
    hipLaunchKernelGGL(aug_resize_post_sharp_grouped_kernel, dim3(tiles, group_len, G), dim3(AUG_T), 0, (hipStream_t)stream, x, y, H, W, table_dev, x,
                       x + (size_t)N * H * W * 3);
    return svla_launch_status();
}
