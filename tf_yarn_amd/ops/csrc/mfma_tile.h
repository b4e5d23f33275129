// Shared pieces of the mfma_f32_16x16x32_bf16 tile kernels (wgrad.hip,
// gemm_bt.hip): the fragment types and the two LDS swizzles.
//
// Fragment maps (guide §3): per lane
//   A[i = lane%16][k = (lane/16)*8 + j],  B[k][m] same shape,
//   C/D col = lane&15, row = (lane>>4)*4 + reg.
// Both operands sit in LDS as [row][64 k] bf16 images, 128 B per row, so a
// fragment is one 16 B read at (row = base + lane%16, k = (lane/16)*8).
#pragma once

#include "common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 mfma_bf16x8;
typedef __attribute__((ext_vector_type(4))) float mfma_f32x4;

// LDS byte offset of element [row n][col k], combined XOR swizzle (v1.5)
// for TRANSPOSED staging (wgrad): (n&7) spreads the b128 READ groups
// (consecutive rows), (n>>3)&7 spreads the b64 WRITE groups (the plain
// (n&7) term made those a 16-way conflict), and the (n>>6) bit-7 term
// splits the write groups across the two 128 B halves of a bank sweep —
// 4-way -> 2-way write conflicts (the 16 B-granular XOR floor for this
// staging shape; verified by bank simulation and PMC
// SQ_LDS_BANK_CONFLICT).  Reads stay at the conflict-free 4 (bit 7 is
// constant across each 16-row read group).
__device__ __forceinline__ int lds_off(int n, int k) {
  int byte = n * 128 + k * 2;
  const int s = ((n ^ (n >> 3)) & 7) | (((n >> 6) & 1) << 3);
  return byte ^ (s << 4);
}

// The same without the bit-7 term, for LINEAR staging (gemm_bt: b128
// writes along k, nothing to split).  A distinct function on purpose.
__device__ __forceinline__ int lds_off_linear(int r, int k) {
  int byte = r * 128 + k * 2;
  return byte ^ (((r ^ (r >> 3)) & 7) << 4);
}
