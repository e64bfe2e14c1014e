// head_dim 96 attention (csrc/attn_hd96.hip): the launchers svla_attn_fwd_bf16 / svla_attn_bwd_bf16 (csrc/attn.hip) dispatch to for head_dim == 96.
// C++ linkage on purpose: these are not entry points of include/svla.h.
#pragma once
#include "common.h"

int attn96_fwd_launch(const bf16_t* Q, const bf16_t* K, const bf16_t* V, long ld, bf16_t* O, long ldo, float* LSE, int rows, int S, int H,
                      float scale, int mask_mode, const int* traj, const float* bias, const unsigned char* kvalid, int Sq, long ldq, int kv_rows,
                      const svla_dropout* drop, void* stream);
int attn96_bwd_launch(const bf16_t* Q, const bf16_t* K, const bf16_t* V, long ld, const bf16_t* O, long ldo, const float* LSE, const bf16_t* dO,
                      long lddo, bf16_t* dQ, bf16_t* dK, bf16_t* dV, long ldd, int rows, int S, int H, float scale, int mask_mode, const int* traj,
                      const float* bias, const unsigned char* kvalid, int Sq, long ldq, long lddq, float* D_ws, const svla_dropout* drop, void* stream);
