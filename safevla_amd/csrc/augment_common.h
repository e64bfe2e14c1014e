// Device code shared by the frame-augmentation kernels: the single-transform launches of augment.hip and the grouped launches of augment_grouped.hip (one
// transform per group of frames, read from a table).  Tile geometry, per-pixel arithmetic, dword-wide staging of byte rows and the index helpers of the blur and
// the resize, moved here from augment.hip as they were.  The arithmetic contract is DESIGN.md "Sampled frame augmentation".
//
// fp contraction is off in every file that includes this: the contract names separate roundings (r*a + (1-r)*b is two products and a sum), and every launch
// form must compute bit for bit what the same stages compute one launch each.
#pragma once
#include "common.h"
#pragma clang fp contract(off)

#define AUG_NPART 64          // partial sums per image (must match ops.AUG_NPART)
#define AUG_CH 2048           // pixels per staged chunk of the gray reduction
#define AUG_TR 16             // tile rows
#define AUG_TC 128            // tile columns (pixels)
#define AUG_T 256             // threads per block

enum { AUG_BRIGHTNESS = 0, AUG_CONTRAST = 1, AUG_SATURATION = 2, AUG_HUE = 3 };      // torchvision ColorJitter's fn_idx codes

struct AugJitter { int nops; int op0, op1, op2, op3; float f0, f1, f2, f3; };
struct AugBlur { int on; float wx0, wx1, wx2, wx3, wx4, wy0, wy1, wy2, wy3, wy4, wy5, wy6, wy7, wy8; };

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
