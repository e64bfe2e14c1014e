// head_dim 64 attention backward for 256 < S <= 512 (csrc/attn_long.hip): the launcher svla_attn_bwd_bf16 (csrc/attn.hip) dispatches to above 256 keys.
// C++ linkage on purpose: this is not an entry point of include/svla.h.
#pragma once
#include "common.h"

int attn_long_bwd_launch(const bf16_t* Q, const bf16_t* K, const bf16_t* V, long ld, const bf16_t* O, long ldo, const float* LSE, const bf16_t* dO,
                         long lddo, bf16_t* dQ, bf16_t* dK, bf16_t* dV, long ldd, int rows, int S, int H, float scale, int mask_mode, const int* traj,
                         const float* bias, const unsigned char* kvalid, int Sq, long ldq, long lddq, float* D_ws, const svla_dropout* drop, void* stream);
