// The tile core of the mfma_f32_16x16x32_bf16 kernels (wgrad.hip,
// gemm_bt.hip, dgrad_drelu.hip): the fragment types, the three LDS images,
// the XCD-grouped tile map, the two register stagings and the k-step.
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

// A lane's place in a fragment: accumulator register r is
// D[row4 + r][col]; an operand fragment is read at row `col`, k = 2 * row4.
__device__ __forceinline__ void frag_pos(int lane, int& col, int& row4) {
  col = lane & 15;
  row4 = (lane >> 4) * 4;
}

template <int FI, int FJ>
__device__ __forceinline__ void zero_acc(mfma_f32x4 (&acc)[FI][FJ]) {
#pragma unroll
  for (int i = 0; i < FI; ++i)
#pragma unroll
    for (int j = 0; j < FJ; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};
}

// Linear block id -> (tile_m, tile_n) of a tiles_m x tiles_n grid.  The
// dispatcher places linear block b on XCD b % 8, so when tiles_m is a
// multiple of 8 the column tiles of one row block take ids sharing b % 8:
// they re-read the SAME operand rows and share them through one XCD's L2
// instead of several.  (wgrad's slab-major (splitk, tiles) grid is a
// different decision and lives in wgrad.hip.)
__device__ __forceinline__ void xcd_tile_map(int tiles_m, int tiles_n,
                                             int& tile_m, int& tile_n) {
  if ((tiles_m & 7) == 0) {
    const int c = blockIdx.x & 7;
    const int q = blockIdx.x >> 3;
    tile_n = q % tiles_n;
    tile_m = c + 8 * (q / tiles_n);
  } else {
    tile_m = blockIdx.x / tiles_n;
    tile_n = blockIdx.x - tile_m * tiles_n;
  }
}

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

// ---- K-major operand staging ([rows][K], K contiguous) ---------------------
// 2 * rows threads cover one [rows][64 k] tile as row = t >> 1,
// k seg = (t & 1) * 32: 32 bf16 per thread per step as four 16 B vectors,
// copied linearly into the image under lds_off_linear.  `p` points at the
// thread's first element and `k` is that element's k index.  K % 16 == 0
// (host check), so whole 8-element vectors are either in or out; a vector
// past K, or any vector of a masked row, is zero and issues no load.
__device__ __forceinline__ void stage_kmajor_load(bf16x8 (&r)[4],
                                                  const unsigned short* p,
                                                  bool row_ok, int k, int K) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    r[c] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    if (row_ok && k + c * 8 + 8 <= K)
      r[c] = *reinterpret_cast<const bf16x8*>(p + c * 8);
  }
}

__device__ __forceinline__ void stage_kmajor_write(unsigned char* img,
                                                   const bf16x8 (&r)[4],
                                                   int row, int k) {
#pragma unroll
  for (int c = 0; c < 4; ++c)
    *reinterpret_cast<bf16x8*>(img + lds_off_linear(row, k + c * 8)) = r[c];
}

// ---- strided-k operand staging ([K][cols], columns contiguous) -------------
// Per tile [64 k][TILE cols] a thread takes 4 k-rows x one oct of columns:
// four coalesced 16 B loads (`p` at the thread's first row, `ld` elements
// between rows), then eight packed b64 transposed writes into a
// [col][64 k] image under lds_off.  Real branches (EXEC-masked loads): a
// masked lane must not issue the load at all (its last row would read past
// the tensor).  `ok` is "column in range and k-rows in range": columns are
// masked by whole octs (cols % 8 == 0) and the thread's four k-rows start
// at a multiple of 4 with K % 4 == 0, so they are all in or all out.
// The register-staged wgrad branch (dy and x) is the load's only caller:
// dgrad_drelu's w operand has it written out (see there) and shares the
// write.
__device__ __forceinline__ void stage_strided_load(bf16x8 (&r)[4],
                                                   const unsigned short* p,
                                                   int64_t ld, bool ok) {
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    r[rr] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    if (ok) r[rr] = *reinterpret_cast<const bf16x8*>(p + rr * ld);
  }
}

union U16x4 {
  unsigned short u[4];
  unsigned long long ll;
};

__device__ __forceinline__ void stage_strided_write(unsigned char* img,
                                                    const bf16x8 (&r)[4],
                                                    int col, int kg) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    U16x4 p{{r[0][j], r[1][j], r[2][j], r[3][j]}};
    *reinterpret_cast<unsigned long long*>(img + lds_off(col + j, kg)) = p.ll;
  }
}

// ---- k-step ---------------------------------------------------------------
// One 64-k step over two [row][64 k] images: per k-half, FI fragments of
// image I from row_i, FJ fragments of image J from row_j (each through its
// image's offset function), then the FI * FJ MFMAs into acc[i][j].  J_FIRST
// hands the J fragment to the MFMA as its first operand: D's row index
// (four consecutive per lane) is then image J's row.
template <int FI, int FJ, int (*OFF_I)(int, int), int (*OFF_J)(int, int),
          bool J_FIRST>
__device__ __forceinline__ void mfma_kstep(mfma_f32x4 (&acc)[FI][FJ],
                                           const unsigned char* img_i,
                                           const unsigned char* img_j,
                                           int row_i, int row_j, int lane) {
  int f_col, f_row4;
  frag_pos(lane, f_col, f_row4);
#pragma unroll
  for (int kh = 0; kh < 2; ++kh) {
    mfma_bf16x8 a[FI], b[FJ];
    const int k = kh * 32 + f_row4 * 2;
#pragma unroll
    for (int i = 0; i < FI; ++i)
      a[i] = *reinterpret_cast<const mfma_bf16x8*>(
          img_i + OFF_I(row_i + i * 16 + f_col, k));
#pragma unroll
    for (int j = 0; j < FJ; ++j)
      b[j] = *reinterpret_cast<const mfma_bf16x8*>(
          img_j + OFF_J(row_j + j * 16 + f_col, k));
#pragma unroll
    for (int i = 0; i < FI; ++i)
#pragma unroll
      for (int j = 0; j < FJ; ++j)
        acc[i][j] = J_FIRST ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                                  b[j], a[i], acc[i][j], 0, 0, 0)
                            : __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                                  a[i], b[j], acc[i][j], 0, 0, 0);
  }
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
