// Host side of the bf16 attention entry points (include/svla.h: svla_attn_fwd_bf16 / svla_attn_bwd_bf16, defined in attn.hip), shared by the translation units of
// the kernel families behind them.  The two entries build ONE record of what the caller passed (AttnCall) and route it on head_dim and S; a family launcher takes that
// record and nothing else.  What a family accepts is one row of data (AttnLimits) read by one check (attn_accepts); what its kernel-argument struct has in common with
// the others' is copied by one function (attn_fill).  A new kernel family adds a row, a launcher declaration and its own one to three fields: it restates none of this.
#pragma once
#include <type_traits>
#include "attn_common.h"      // MASK_*, DropCfg

// The arguments of svla_attn_fwd_bf16 / svla_attn_bwd_bf16 as the caller gave them (defaults not yet applied); head_dim is spent on the routing.
// The forward leaves the gradient fields (dO .. ldd, lddq, D_ws) zero; the backward leaves kv_rows zero and only reads O and LSE.
struct AttnCall {
    const bf16_t *Q, *K, *V; long ld;
    bf16_t* O; long ldo;
    float* LSE;
    const bf16_t* dO; long lddo;
    bf16_t *dQ, *dK, *dV; long ldd;
    int rows, S, H;
    float scale;
    int mask_mode;
    const int* traj;
    const float* bias;
    const unsigned char* kvalid;
    int Sq; long ldq, lddq;      // Sq == 0: all S queries, Q / dQ on the K/V strides
    int kv_rows;                 // <= 0: S
    float* D_ws;
    const svla_dropout* drop;
    hipStream_t stream;
};

#define DEC_MAXS 1024      // keys of the longest cache window or KV ring (the LDS score arrays of attn_decode.hip)

// What one kernel family takes.  Every family also needs rows, H > 0, 0 <= Sq <= S, ld % 8 == 0, lddo % 8 == 0, Sq > 0 ? ldq % 8 == 0, kv_rows <= 0 or >= S, and
// traj with the block-causal mask.  (A stride the call does not have is 0 and passes any multiple.)
struct AttnLimits {
    int s_min, s_max;
    bool bias_ok;               // the additive T5 bias
    bool known_masks_only;      // refuse mask_mode values other than MASK_NONE / MASK_BLOCK_CAUSAL (false: they run as "no trajectory mask")
    int ldo_mult, ldd_mult, lddq_mult;
};
//                                                   S              bias   masks  ldo ldd lddq
constexpr AttnLimits ATTN_FWD_64          = {  1,       512, true,  false, 1, 1, 1};      // attn.hip: the tile kernels
constexpr AttnLimits ATTN_FWD_64_DECODE   = {  1,  DEC_MAXS, false, true,  1, 1, 1};      // attn_decode.hip: what svla_attn_fwd_bf16 routes there (one query, no bias / mask / dropout)
constexpr AttnLimits ATTN_FWD_64_CAUSAL_L = {  1,  DEC_MAXS, false, true,  8, 1, 1};      // attn_seq_long.hip: its own entry (svla_attn_causal_fwd_bf16), which also asks for ld, ldo >= H * 64
constexpr AttnLimits ATTN_FWD_96          = {  1,       256, false, true,  4, 1, 1};      // attn_hd96.hip
constexpr AttnLimits ATTN_BWD_64          = {  1,       256, true,  false, 1, 1, 8};      // attn.hip
constexpr AttnLimits ATTN_BWD_64_LONG     = {257,       512, false, true,  8, 4, 4};      // attn_long.hip
constexpr AttnLimits ATTN_BWD_96          = {  1,       256, false, true,  8, 4, 4};      // attn_hd96.hip

inline bool attn_accepts(const AttnCall& c, const AttnLimits& m) {
    if (c.rows <= 0 || c.H <= 0 || c.S < m.s_min || c.S > m.s_max || (c.bias && !m.bias_ok)) return false;
    if (m.known_masks_only && c.mask_mode != MASK_NONE && c.mask_mode != MASK_BLOCK_CAUSAL) return false;
    if (c.mask_mode == MASK_BLOCK_CAUSAL && !c.traj) return false;
    if (c.Sq < 0 || c.Sq > c.S || (c.Sq > 0 && ((c.ldq % 8) || (c.lddq % m.lddq_mult)))) return false;
    if ((c.ld % 8) || (c.lddo % 8) || (c.ldo % m.ldo_mult) || (c.ldd % m.ldd_mult)) return false;
    return c.kv_rows <= 0 || c.kv_rows >= c.S;
}

// The fields AttnArgs, Attn96Args and AttnLongArgs share, defaults applied; the rest of Args is zero (a family then sets what only it has: bias, kv_rows, Dws)
template <class Args> inline Args attn_fill(const AttnCall& c) {
    Args p{};
    p.Q = c.Q; p.K = c.K; p.V = c.V; p.ld = c.ld; p.O = c.O; p.ldo = c.ldo; p.LSE = c.LSE; p.dO = c.dO; p.lddo = c.lddo;
    p.dQ = c.dQ; p.dK = c.dK; p.dV = c.dV; p.ldd = c.ldd; p.traj = c.traj; p.kvalid = c.kvalid;
    p.S = c.S; p.H = c.H; p.mask_mode = c.mask_mode; p.scale = c.scale;
    p.Sq = c.Sq > 0 ? c.Sq : c.S; p.ldq = c.Sq > 0 ? c.ldq : c.ld; p.lddq = c.Sq > 0 ? c.lddq : c.ldd;
    p.drop = drop_cfg(c.drop);
    return p;
}
inline int attn_kv_rows(const AttnCall& c) { return c.kv_rows > 0 ? c.kv_rows : c.S; }

// f(std::integral_constant<int, N>) for the first N of the list whose N 16-key tiles hold S keys; the last N takes what is left (the caller has checked that it fits)
template <int N0, int... N, class F> inline int attn_bucket(int S, F&& f) {
    if constexpr (sizeof...(N) == 0) return f(std::integral_constant<int, N0>{});
    else return S <= N0 * 16 ? f(std::integral_constant<int, N0>{}) : attn_bucket<N...>(S, f);
}

// ---- the family launchers (C++ linkage: not entry points of include/svla.h); each refuses with SVLA_EINVAL what its row above does not take
int attn96_fwd_launch(const AttnCall& c);            // attn_hd96.hip: head_dim 96
int attn96_bwd_launch(const AttnCall& c);
int attn_long_bwd_launch(const AttnCall& c);         // attn_long.hip: head_dim 64, 256 < S <= 512 (D_ws is accepted and unused: the dK/dV kernel computes D itself)
int attn_decode_launch(const AttnCall& c);           // attn_decode.hip: head_dim 64, one query, S <= DEC_MAXS
