// Shared pieces of the mfma_f32_16x16x32_bf16 tile kernels (wgrad.hip,
// gemm_bt.hip): the fragment types and the three LDS images.
//
// Fragment maps (guide §3): per lane
//   A[i = lane%16][k = (lane/16)*8 + j],  B[k][m] same shape,
//   C/D col = lane&15, row = (lane>>4)*4 + reg.
// In the first two images both operands sit in LDS as [row][64 k] bf16,
// 128 B per row, so a fragment is one 16 B read at (row = base + lane%16,
// k = (lane/16)*8); the third keeps k as the row and is read transposed.
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

// Third image, for operands whose k axis is the STRIDED one (wgrad's dy
// and x, both [batch][features]) staged by LDS-DMA: [64 k-rows][128
// columns] bf16 with plain 256 B rows, 16 KB, never transposed on the way
// in.  lds_off_tr is the byte offset of 16 B chunk ch (0..15) of k-row
// row (guide T10, image (b)).  An LDS-DMA wave-instruction writes 1 KB =
// four rows lane-linearly, so the XOR goes on the per-lane SOURCE address
// (lane L fetches logical chunk (L%16) ^ lds_swz_tr(row) of row
// r0 + L/16); fragments come out of it through ds_read_b64_tr_b16, two
// per mfma_bf16x8: lane 4q+p of a 16-lane group supplies
// lds_off_tr(r0 + q, 2c + (p>>1)) + 8*(p&1) for the 4-row block r0 of
// columns 16c..16c+15 and lane i receives column i, row q in element q.
// A half-wave's two blocks sit 8 rows apart in the same columns: by the
// bank rule ((a/4) % 64 per 32-lane half) the reads are conflict-free.
// Host-callable too: wgrad_glds_layout() reports the table to the tests.
__host__ __device__ constexpr int lds_swz_tr(int row) {
  return ((row & 3) << 2) | ((row >> 2) & 3);
}
__host__ __device__ constexpr int lds_off_tr(int row, int ch) {
  return 256 * row + 16 * (ch ^ lds_swz_tr(row));
}
