// head_dim 64 single-query ("decode") attention forward for 512 < S <= 1024 (csrc/attn_decode_long.hip): the launcher svla_attn_fwd_bf16 (csrc/attn.hip)
// dispatches to it above 512 keys.  C++ linkage on purpose: this is not an entry point of include/svla.h.
#pragma once
#include "common.h"

#define DECL_MAXS 1024

int attn_decode_long_launch(const bf16_t* Q, const bf16_t* K, const bf16_t* V, long ld, bf16_t* O, long ldo, float* LSE, int rows, int S, int H, float scale,
                            const unsigned char* kvalid, long ldq, int kv_rows, void* stream);
