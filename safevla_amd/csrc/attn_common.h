// Device primitives shared by the attention translation units (attn.hip, attn_long.hip, attn_hd96.hip, attn_fp8.hip, attn_decode.hip).  Two of them are
// contracts between files: the dropout element index decides WHICH probabilities are dropped (forward, backward, the fp8 variant and the fp32 twin of f32.hip
// must agree bit for bit), and the chunk swizzle is the LDS image that staging stores and both kinds of fragment read share.  A new attention kernel includes
// this header; it does not copy from it.
#pragma once
#include "common.h"

static constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;

enum { MASK_NONE = 0, MASK_BLOCK_CAUSAL = 1 };      // mask_mode of the svla_attn_* entry points (include/svla.h)

// element index of probability (row r, head h, query q, key k): ((r*H + h)*S + q) * SP4 + k with the key stride SP4 = S rounded
// up to a multiple of 4, so that the 4 consecutive keys a lane holds share two RNG words (include/svla.h: svla_dropout)
__device__ __forceinline__ unsigned long long att_drop_row(int S, int H, int r, int h, int q) {
    return ((unsigned long long)((size_t)r * H + h) * S + q) * (unsigned long long)((S + 3) & ~3);
}
__device__ __forceinline__ bool att_keep1(const DropCfg& c, unsigned long long e) {
    const unsigned x = drop_bits(c.key, e >> 1);
    return ((e & 1) ? (x >> 16) : (x & 0xffffu)) >= c.thr;
}

// ---- LDS image of a 64-wide head slice: rows of LDSROW bf16 = 128 B = eight 16-byte chunks, XOR-swizzled
#define LDSROW 64

// physical 16-byte chunk of logical chunk c in row r: c ^ f(x), x = (r >> 1) & 7 (64 banks x 4 B; a row is 32 banks, so the row
// parity picks the bank half and f only has to spread the eight values of x over the eight 16-byte slots of a half).  Three
// access patterns constrain f:
//  * ds_read_b128 row fragments (row = lane & 15, logical chunk = lane >> 4): the hardware serves lanes {0-3,12-15,20-27},
//    {4-11,16-19,28-31}, ... as groups, i.e. rows with x in {0,1,6,7} on chunk c together with rows with x in {2,3,4,5} on
//    chunk c ^ 1: conflict-free iff f is a permutation and f({2,3,4,5}) is a union of two chunk pairs {2k, 2k+1};
//  * ds_read_b64_tr_b16 (32 lanes per pass = 8 rows x 32 B = one chunk PAIR per row): f >> 1 must be distinct over
//    x = 0..3 and over x = 4..7.  (f = x, the first layout, put rows 2,3 on the chunk pair of rows 0,1: every transposed
//    read was a 2-way conflict.)
//  * staging stores (8 lanes = one row): any f.
// f = 0,2,4,6,5,7,1,3 satisfies all three.  (Panel A of the 96-wide image of attn_hd96.hip is this layout too.)
__device__ __forceinline__ int att_swz(int row) {
    const int x = (row >> 1) & 7;
    return (((x + ((x >> 2) << 1)) & 3) << 1) | (x >> 2);
}

// Lane bases of the two access patterns (tile rows are multiples of 16, so the swizzle term depends on the lane only and the
// tile offset stays a compile-time immediate of the ds_read):
//   row fragment  : row = tile + (lane & 15), logical chunk (lane >> 4) [+4 for columns 32..63]
//   transposed    : row = tile + 4 (lane >> 4) + ((lane & 15) >> 2), columns dt*16 + 4 ((lane & 15) & 3) .. +3
struct RowBase { const bf16_t* lo; const bf16_t* hi; };
__device__ __forceinline__ RowBase att_row_base(const bf16_t* tile, int lane) {
    const int ql = lane & 15, g = lane >> 4, f = att_swz(ql);
    return RowBase{tile + ql * LDSROW + ((g ^ f) << 3), tile + ql * LDSROW + (((g + 4) ^ f) << 3)};
}
struct TrBase { const bf16_t* d[4]; };
__device__ __forceinline__ TrBase att_tr_base(const bf16_t* tile, int lane) {
    const int ql = lane & 15, g = lane >> 4;
    const int row = 4 * g + (ql >> 2), f = att_swz(row);
    TrBase t;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) t.d[dt] = tile + row * LDSROW + (((2 * dt + ((ql & 3) >> 1)) ^ f) << 3) + 4 * (ql & 1);
    return t;
}
__device__ __forceinline__ bf16x8 lds_row8i(const bf16_t* lane_base, int tile_row0) {
    return *(const bf16x8*)(lane_base + tile_row0 * LDSROW);
}
// B/A-operand gather: 8 reduction slots = rows {rA + 4g + 0..3, rB + 4g + 0..3}, column dt*16 + (lane & 15)
__device__ __forceinline__ bf16x8 lds_tr8i(const bf16_t* lane_base_dt, int rA, int rB) {
    const bf16x4 lo = lds_tr16_b64(lane_base_dt + rA * LDSROW);
    const bf16x4 hi = lds_tr16_b64(lane_base_dt + rB * LDSROW);
    return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// ---- register fragments
__device__ __forceinline__ bf16x8 pack8(const float (&v)[8]) {
    u32x4 w;
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = pack_bf2(v[2 * i], v[2 * i + 1]);
    return __builtin_bit_cast(bf16x8, w);
}
// 16-byte global load of 8 bf16, zeros when !ok (p is not dereferenced then)
__device__ __forceinline__ bf16x8 gld8(const bf16_t* p, bool ok) { return ok ? *(const bf16x8*)p : bf16x8{0, 0, 0, 0, 0, 0, 0, 0}; }
__device__ __forceinline__ float dot8(bf16x8 a, bf16x8 b) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += bf2f((bf16_t)a[i]) * bf2f((bf16_t)b[i]);
    return s;
}

// key `key` is hidden from query q (Args: any args struct with S and mask_mode; traj_s / kv_s: the row's trajectory ids and key-validity bytes, kv_s may be null)
template <class Args>
__device__ __forceinline__ bool att_masked(const Args& p, int q, int key, const int* traj_s, const unsigned char* kv_s) {
    if (key >= p.S) return true;
    if (p.mask_mode == MASK_BLOCK_CAUSAL && (key > q || traj_s[key] != traj_s[q])) return true;
    if (kv_s && !kv_s[key]) return true;
    return false;
}
