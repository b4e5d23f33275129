// The Compressed Interaction Network layer of xDeepFM for MI355X, bf16,
// forward and backward, without the [B, H_in*m, D] outer-product tensor.
//
// m fields, embedding width D, H_in input maps, H_out output maps; all 2-D
// row-major bf16: x0 [B, m*D] (field j at columns j*D ..), x [B, H_in*D],
// weight [H_out, H_in, m], y [B, H_out*D].  Products and sums are fp32:
//
//   z[b,i,j,c] = bf16(x[b,i,c] * x0[b,j,c])                 (one rounding)
//   y[b,h,c]   = bf16(sum_{i,j} W[h,i,j] * z[b,i,j,c])      (one rounding)
//
// Backward with g = grad_y (the rounding of z is the identity):
//
//   dU[b,i,j,c] = sum_h g[b,h,c] * W[h,i,j]      (fp32, never stored)
//   dx[b,i,c]   = bf16(sum_j dU * x0[b,j,c])
//   dx0[b,j,c]  = bf16(sum_i dU * x[b,i,c])
//   dW[h,i,j]   = bf16(sum_{b,c} g[b,h,c] * z[b,i,j,c])    (the forward's z)
//
// GEMM view: the rows are the (b, c) pairs, so the 16 columns of one D-chunk
// of one example are one 16-row M tile ("item" = b * D/16 + chunk); N is
// H_out; K is the (i, j) pairs with j padded to MP = 32, so one
// mfma_f32_16x16x32_bf16 k-step is one input map i and all fields.
//
//  * Forward: a wave owns CIN_MT = 4 items by up to 8 N tiles (128 output
//    maps; H_out = 256 makes two passes).  Lane l is column c = l%16 and
//    field group q = l/16 of its items: it keeps x0[b, 8q..8q+7, c] as eight
//    floats for the whole k-loop, reads one x[b,i,c] per k-step from the
//    block's LDS image, forms the eight products, rounds each once (packed
//    converts) and has the A fragment; every N tile reuses it.  The B
//    fragment W[h = 16t + l%16][i][8q..8q+7] is one 16 B read of a chunk of
//    CIN_IC input maps of a PACKED copy of W, [H_in][H_out][32] with the
//    fields >= m zero (cin_pack_kernel, once per call), staged linearly as
//    [ic][h][32]: a wave reads 1 KB in a row.  The accumulator gives a lane
//    four consecutive c of one h: at D = 16 a wave stores 512 B in a row.
//  * Data backward: the same items.  Per input map i the [32 j x 16 c] tile
//    dU^T = W_i^T g^T is two MFMA tiles contracted over h (H_out padded to
//    32s with zeros).  The lane's g fragments (g[b, 32s + 8q + 0..7, c]) do
//    not depend on i and stay in registers for the whole i loop; W_i^T comes
//    from a second packed copy, [H_in][32][Hpad], staged with 16 B of row
//    padding.  The accumulator holds dU[j = 16jt + 4q + r][c]:
//    dx0 += dU * x[b,i,c] in registers over the i loop, dx[i][c] is the
//    in-lane sum over the lane's eight j and two exchanges over q.
//  * Weight gradient: all operands are contiguous in c.  Output tile
//    [16 h x (i, 16 fields)], contraction over the flat (b, c) index, 32 per
//    k-step; A = g[b, h, c0..c0+7] is a 16 B load, B = bf16(x * x0) of two
//    16 B loads.  A wave owns 4 (i, field-half) tiles by up to 8 h tiles;
//    the grid is tile blocks x batch splits x 128-wide h blocks; each split
//    writes an fp32 partial and cin_reduce_kernel sums them in split order
//    and rounds once: no atomics, the same bits every call.
//
// Every block makes whole trips, so its barriers are uniform; dead items
// compute on zeros and store nothing.  An example's values meet no other
// example's in the forward and the data backward.  m > 32, fp32, bias and
// activation are not built.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include "mfma_tile.h"
#include <algorithm>
#include <vector>

namespace {

typedef __attribute__((ext_vector_type(2))) float cin_f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 cin_bf16x2;

constexpr int CIN_WAVES = MIYARN_BLOCK / 64;
constexpr int CIN_MP = 32;       // the fields, padded
constexpr int CIN_MAX_H = 256;   // input and output maps
constexpr int CIN_MT = 4;        // items of a wave (forward)
constexpr int CIN_NT = 8;        // N tiles of a pass: 128 maps
constexpr int CIN_IC = 4;        // input maps of a staged chunk (forward)
constexpr int CIN_WG_NT = 4;     // (i, field-half) tiles of a wave (dW)
constexpr int CIN_MAX_SPLITS = 32;

// bf16(a[e] * b[e]), e = 0..7: fp32 products, each rounded once to nearest
// even by the packed convert.
__device__ __forceinline__ mfma_bf16x8 product_frag(const float (&a)[8],
                                                    const float (&b)[8]) {
  mfma_bf16x8 z;
#pragma unroll
  for (int e = 0; e < 8; e += 2) {
    const cin_f32x2 p = {a[e] * b[e], a[e + 1] * b[e + 1]};
    const cin_bf16x2 r = __builtin_convertvector(p, cin_bf16x2);
    z[e] = r[0];
    z[e + 1] = r[1];
  }
  return z;
}

__device__ __forceinline__ void unpack8(bf16x8 v, float (&f)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = bf16_to_f32(v[e]);
}

__device__ __forceinline__ float lane_xor(float v, int lane, int mask) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_ds_bpermute((lane ^ mask) << 2,
                                          __builtin_bit_cast(int, v)));
}

// The two packed copies of W.  transposed = false: [H_in][H_out][32] (the
// forward's B fragments); true: [H_in][32][hpad] (the data backward's A
// fragments).  Fields >= m and maps >= H_out are zeros.
__global__ __launch_bounds__(MIYARN_BLOCK) void
cin_pack_kernel(const unsigned short* __restrict__ w,
                unsigned short* __restrict__ out, int m, int H_in, int H_out,
                int hpad, bool transposed) {
  const int per_i = CIN_MP * (transposed ? hpad : H_out);
  const int total = H_in * per_i;
  for (int idx = blockIdx.x * MIYARN_BLOCK + threadIdx.x; idx < total;
       idx += gridDim.x * MIYARN_BLOCK) {
    const int i = idx / per_i, rem = idx - i * per_i;
    const int h = transposed ? rem % hpad : rem / CIN_MP;
    const int j = transposed ? rem / hpad : rem % CIN_MP;
    out[idx] = (j < m && h < H_out) ? w[((int64_t)h * H_in + i) * m + j] : 0;
  }
}

__global__ __launch_bounds__(MIYARN_BLOCK) void
cin_fwd_kernel(const unsigned short* __restrict__ x0,
               const unsigned short* __restrict__ x,
               const unsigned short* __restrict__ wp,
               unsigned short* __restrict__ y, int64_t items, int m, int H_in,
               int H_out, int D, int64_t ld0, int64_t ldx) {
  __shared__ __attribute__((aligned(16))) unsigned short
      w_img[CIN_IC * 16 * CIN_NT * CIN_MP];
  __shared__ __attribute__((aligned(16))) unsigned short
      x_img[CIN_WAVES * CIN_MT * CIN_IC * 16];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int KC = D >> 4;
  constexpr int TRIP = CIN_WAVES * CIN_MT;
  // the thread's 16 B of the x image: item tid/8, map (tid/2)%4, half tid%2
  const int s_ic = (tid >> 1) & (CIN_IC - 1);

  for (int64_t base = (int64_t)blockIdx.x * TRIP; base < items;
       base += (int64_t)gridDim.x * TRIP) {
    float x0f[CIN_MT][8];
    int64_t b_of[CIN_MT];
    int cc_of[CIN_MT];
    bool live[CIN_MT];
#pragma unroll
    for (int t = 0; t < CIN_MT; ++t) {
      const int64_t item = base + wave * CIN_MT + t;
      live[t] = item < items;
      b_of[t] = item / KC;
      cc_of[t] = (int)(item - b_of[t] * KC);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int j = 8 * q + e;
        x0f[t][e] = 0.f;
        if (live[t] && j < m)
          x0f[t][e] = bf16_to_f32(
              x0[b_of[t] * ld0 + j * D + 16 * cc_of[t] + c]);
      }
    }
    const int64_t s_item = base + (tid >> 3);
    const bool s_live = tid < TRIP * CIN_IC * 2 && s_item < items;
    const int64_t s_b = s_item / KC;
    const unsigned short* s_src =
        x + s_b * ldx + 16 * (int)(s_item - s_b * KC) + 8 * (tid & 1);

    for (int nb0 = 0; nb0 < H_out; nb0 += 16 * CIN_NT) {
      const int nh = min(16 * CIN_NT, H_out - nb0);
      const int nt = nh >> 4;
      mfma_f32x4 acc[CIN_MT][CIN_NT];
      zero_acc<CIN_MT, CIN_NT>(acc);
      for (int i0 = 0; i0 < H_in; i0 += CIN_IC) {
        const int icn = min(CIN_IC, H_in - i0);
        __syncthreads();  // the images' readers are done
        const int per_ic = nh * (CIN_MP / 8);
        for (int v = tid; v < icn * per_ic; v += MIYARN_BLOCK) {
          const int ic = v / per_ic;
          *reinterpret_cast<bf16x8*>(w_img + v * 8) =
              *reinterpret_cast<const bf16x8*>(
                  wp + ((int64_t)(i0 + ic) * H_out + nb0) * CIN_MP +
                  (v - ic * per_ic) * 8);
        }
        if (tid < TRIP * CIN_IC * 2) {
          bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
          if (s_live && s_ic < icn)
            v = *reinterpret_cast<const bf16x8*>(s_src + (i0 + s_ic) * D);
          *reinterpret_cast<bf16x8*>(x_img + tid * 8) = v;
        }
        __syncthreads();
        for (int ic = 0; ic < icn; ++ic) {
          mfma_bf16x8 a[CIN_MT];
#pragma unroll
          for (int t = 0; t < CIN_MT; ++t) {
            const float xv = bf16_to_f32(
                x_img[((wave * CIN_MT + t) * CIN_IC + ic) * 16 + c]);
            const float xs[8] = {xv, xv, xv, xv, xv, xv, xv, xv};
            a[t] = product_frag(xs, x0f[t]);
          }
#pragma unroll
          for (int n = 0; n < CIN_NT; ++n) {
            if (n >= nt) continue;
            const mfma_bf16x8 b = *reinterpret_cast<const mfma_bf16x8*>(
                w_img + (ic * nh + 16 * n + c) * CIN_MP + 8 * q);
#pragma unroll
            for (int t = 0; t < CIN_MT; ++t)
              acc[t][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  a[t], b, acc[t][n], 0, 0, 0);
          }
        }
      }
      // register r of lane (q, l%16): c = 4q + r of map nb0 + 16n + l%16
#pragma unroll
      for (int t = 0; t < CIN_MT; ++t) {
        if (!live[t]) continue;
        unsigned short* dst = y + b_of[t] * ((int64_t)H_out * D) +
                              (int64_t)(nb0 + c) * D + 16 * cc_of[t] + 4 * q;
#pragma unroll
        for (int n = 0; n < CIN_NT; ++n) {
          if (n >= nt) continue;
          bf16x4 v;
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = f32_to_bf16(acc[t][n][r]);
          *reinterpret_cast<bf16x4*>(dst + 16 * n * D) = v;
        }
      }
    }
  }
}

// KS: the 32-wide steps over h the g fragments are held for; MT: the items
// of a wave; 16 / KS input maps per staged chunk.  LDS: the W^T chunk
// [IC][32][32*ks + 8], then the x image [4*MT][IC][16].
template <int KS, int MT>
__global__ __launch_bounds__(MIYARN_BLOCK) void
cin_bwd_data_kernel(const unsigned short* __restrict__ g,
                    const unsigned short* __restrict__ x0,
                    const unsigned short* __restrict__ x,
                    const unsigned short* __restrict__ wt,
                    unsigned short* __restrict__ dx,
                    unsigned short* __restrict__ dx0, int64_t items, int m,
                    int H_in, int H_out, int D, int64_t ldg, int64_t ld0,
                    int64_t ldx) {
  constexpr int IC = 16 / KS;
  constexpr int TRIP = CIN_WAVES * MT;
  extern __shared__ __attribute__((aligned(16))) unsigned short cin_lds[];
  const int ks = (H_out + 31) >> 5;
  const int hpad = 32 * ks, pitch = hpad + 8;
  unsigned short* w_img = cin_lds;
  unsigned short* x_img = cin_lds + IC * CIN_MP * pitch;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int KC = D >> 4;
  const int jtn = m > 16 ? 2 : 1;
  const int s_ic = (tid >> 1) % IC;

  for (int64_t base = (int64_t)blockIdx.x * TRIP; base < items;
       base += (int64_t)gridDim.x * TRIP) {
    mfma_bf16x8 gf[MT][KS];
    float x0f[MT][2][4];
    mfma_f32x4 dx0acc[MT][2];
    int64_t b_of[MT];
    int cc_of[MT];
    bool live[MT];
    zero_acc<MT, 2>(dx0acc);
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      const int64_t item = base + wave * MT + t;
      live[t] = item < items;
      b_of[t] = item / KC;
      cc_of[t] = (int)(item - b_of[t] * KC);
      const int col = 16 * cc_of[t] + c;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int h = 32 * s + 8 * q + e;
          if (live[t] && h < H_out) v[e] = g[b_of[t] * ldg + h * D + col];
        }
        gf[t][s] = __builtin_bit_cast(mfma_bf16x8, v);
      }
#pragma unroll
      for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = 16 * jt + 4 * q + r;
          x0f[t][jt][r] = 0.f;
          if (live[t] && j < m)
            x0f[t][jt][r] = bf16_to_f32(x0[b_of[t] * ld0 + j * D + col]);
        }
    }
    const int64_t s_item = base + tid / (IC * 2);
    const bool s_live = tid < TRIP * IC * 2 && s_item < items;
    const int64_t s_b = s_item / KC;
    const unsigned short* s_src =
        x + s_b * ldx + 16 * (int)(s_item - s_b * KC) + 8 * (tid & 1);

    for (int i0 = 0; i0 < H_in; i0 += IC) {
      const int icn = min(IC, H_in - i0);
      __syncthreads();  // the images' readers are done
      const int per_row = hpad >> 3;
      for (int v = tid; v < icn * CIN_MP * per_row; v += MIYARN_BLOCK) {
        const int row = v / per_row, col8 = v - row * per_row;
        *reinterpret_cast<bf16x8*>(w_img + row * pitch + col8 * 8) =
            *reinterpret_cast<const bf16x8*>(
                wt + ((int64_t)i0 * CIN_MP + row) * hpad + col8 * 8);
      }
      if (tid < TRIP * IC * 2) {
        bf16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (s_live && s_ic < icn)
          v = *reinterpret_cast<const bf16x8*>(s_src + (i0 + s_ic) * D);
        *reinterpret_cast<bf16x8*>(x_img + tid * 8) = v;
      }
      __syncthreads();
      for (int ic = 0; ic < icn; ++ic) {
        // dU^T = W_i^T g^T: register r of tile jt is field 16jt + 4q + r
        mfma_f32x4 du[MT][2];
        zero_acc<MT, 2>(du);
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          if (s >= ks) continue;
#pragma unroll
          for (int jt = 0; jt < 2; ++jt) {
            if (jt >= jtn) continue;
            const mfma_bf16x8 a = *reinterpret_cast<const mfma_bf16x8*>(
                w_img + (ic * CIN_MP + 16 * jt + c) * pitch + 32 * s + 8 * q);
#pragma unroll
            for (int t = 0; t < MT; ++t)
              du[t][jt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  a, gf[t][s], du[t][jt], 0, 0, 0);
          }
        }
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          const float xv =
              bf16_to_f32(x_img[((wave * MT + t) * IC + ic) * 16 + c]);
          float sum = 0.f;
#pragma unroll
          for (int jt = 0; jt < 2; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              dx0acc[t][jt][r] += du[t][jt][r] * xv;
              sum += du[t][jt][r] * x0f[t][jt][r];
            }
          sum += lane_xor(sum, lane, 16);
          sum += lane_xor(sum, lane, 32);
          if (q == 0 && live[t])
            dx[b_of[t] * ((int64_t)H_in * D) + (int64_t)(i0 + ic) * D +
               16 * cc_of[t] + c] = f32_to_bf16(sum);
        }
      }
    }
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int j = 16 * jt + 4 * q + r;
          if (live[t] && j < m)
            dx0[b_of[t] * ((int64_t)m * D) + j * D + 16 * cc_of[t] + c] =
                f32_to_bf16(dx0acc[t][jt][r]);
        }
  }
}

// grid (tile blocks, splits, 128-wide h blocks); part [splits][H_out][H_in]
// [32] fp32.  k-step s of the flat (b, c) index covers 32s .. 32s + 31; a
// lane's eight, 32s + 8q + 0..7, lie in one example (D % 16 == 0).
__global__ __launch_bounds__(MIYARN_BLOCK) void
cin_bwd_weight_kernel(const unsigned short* __restrict__ g,
                      const unsigned short* __restrict__ x0,
                      const unsigned short* __restrict__ x,
                      float* __restrict__ part, int64_t total_k,
                      int64_t steps_per_split, int m, int H_in, int H_out,
                      int D, int64_t ldg, int64_t ld0, int64_t ldx) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int jtn = m > 16 ? 2 : 1;
  const int tiles = H_in * jtn;
  const int hb0 = blockIdx.z * 16 * CIN_NT;
  const int htn = min(CIN_NT, (H_out - hb0) >> 4);
  int i_of[CIN_WG_NT], j_of[CIN_WG_NT];
  bool ok[CIN_WG_NT];
#pragma unroll
  for (int t = 0; t < CIN_WG_NT; ++t) {
    const int tile = (blockIdx.x * CIN_WAVES + wave) * CIN_WG_NT + t;
    ok[t] = tile < tiles;
    i_of[t] = tile / jtn;
    j_of[t] = 16 * (tile - i_of[t] * jtn) + c;
  }
  mfma_f32x4 acc[CIN_WG_NT][CIN_NT];
  zero_acc<CIN_WG_NT, CIN_NT>(acc);
  const int64_t steps = (total_k + 31) >> 5;
  const int64_t s0 = blockIdx.y * steps_per_split;
  const int64_t s1 = min(s0 + steps_per_split, steps);
  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int64_t s = s0; s < s1; ++s) {
    const int64_t kk = 32 * s + 8 * q;
    const bool in = kk < total_k;
    const int64_t b = kk / D;
    const int col = (int)(kk - b * D);
    mfma_bf16x8 a[CIN_NT];
#pragma unroll
    for (int ht = 0; ht < CIN_NT; ++ht) {
      bf16x8 v = zero8;
      if (in && ht < htn)
        v = *reinterpret_cast<const bf16x8*>(
            g + b * ldg + (hb0 + 16 * ht + c) * D + col);
      a[ht] = __builtin_bit_cast(mfma_bf16x8, v);
    }
#pragma unroll
    for (int t = 0; t < CIN_WG_NT; ++t) {
      if (!ok[t]) continue;  // the whole wave
      bf16x8 xv = zero8, x0v = zero8;
      if (in) {
        xv = *reinterpret_cast<const bf16x8*>(x + b * ldx + i_of[t] * D + col);
        if (j_of[t] < m)
          x0v = *reinterpret_cast<const bf16x8*>(
              x0 + b * ld0 + j_of[t] * D + col);
      }
      float xf[8], x0f[8];
      unpack8(xv, xf);
      unpack8(x0v, x0f);
      const mfma_bf16x8 z = product_frag(xf, x0f);
#pragma unroll
      for (int ht = 0; ht < CIN_NT; ++ht) {
        if (ht >= htn) continue;
        acc[t][ht] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a[ht], z, acc[t][ht], 0, 0, 0);
      }
    }
  }
  // register r of lane (q, l%16): map hb0 + 16ht + 4q + r, field j_of
#pragma unroll
  for (int t = 0; t < CIN_WG_NT; ++t) {
    if (!ok[t]) continue;
#pragma unroll
    for (int ht = 0; ht < CIN_NT; ++ht) {
      if (ht >= htn) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int h = hb0 + 16 * ht + 4 * q + r;
        part[(((int64_t)blockIdx.y * H_out + h) * H_in + i_of[t]) * CIN_MP +
             j_of[t]] = acc[t][ht][r];
      }
    }
  }
}

// dW[h][i][j] = bf16(part[0] + part[1] + ...), in split order.
__global__ __launch_bounds__(MIYARN_BLOCK) void
cin_reduce_kernel(const float* __restrict__ part,
                  unsigned short* __restrict__ dw, int splits, int m,
                  int rows /* H_out * H_in */) {
  const int total = rows * m;
  for (int idx = blockIdx.x * MIYARN_BLOCK + threadIdx.x; idx < total;
       idx += gridDim.x * MIYARN_BLOCK) {
    const int row = idx / m, j = idx - row * m;
    float sum = 0.f;
    for (int s = 0; s < splits; ++s)
      sum += part[((int64_t)s * rows + row) * CIN_MP + j];
    dw[idx] = f32_to_bf16(sum);
  }
}

// [rows, cols] bf16 with unit column stride, rows a multiple of 8 elements
// and at least their own width apart and a 16 B aligned base.
bool rows_vector_ok(const torch::Tensor& t) {
  return t.is_cuda() && t.dim() == 2 &&
         t.scalar_type() == torch::kBFloat16 &&
         (t.size(1) <= 1 || t.stride(1) == 1) &&
         (t.size(0) <= 1 ||
          (t.stride(0) >= t.size(1) && t.stride(0) % 8 == 0)) &&
         miyarn_aligned(t.data_ptr(), 16);
}

int64_t row_ld(const torch::Tensor& t) {
  return t.size(0) > 1 ? t.stride(0) : t.size(1);
}

// The embedding width the kernels take for these operands, or 0.
int64_t cin_width(const torch::Tensor& x0, const torch::Tensor& x,
                  const torch::Tensor& w) {
  if (!rows_vector_ok(x0) || !rows_vector_ok(x) || !w.is_cuda() ||
      w.scalar_type() != torch::kBFloat16 || w.dim() != 3 ||
      !w.is_contiguous() || x0.device() != x.device() ||
      x0.device() != w.device() || x0.size(0) != x.size(0))
    return 0;
  const int64_t H_out = w.size(0), H_in = w.size(1), m = w.size(2);
  if (m < 2 || m > CIN_MP || H_in < 1 || H_in > CIN_MAX_H || H_out < 16 ||
      H_out > CIN_MAX_H || H_out % 16 != 0 || x0.size(1) % m != 0)
    return 0;
  const int64_t d = x0.size(1) / m;
  return (d == 16 || d == 32 || d == 64) && x.size(1) == H_in * d ? d : 0;
}

int64_t checked_width(const torch::Tensor& x0, const torch::Tensor& x,
                      const torch::Tensor& w) {
  const int64_t d = cin_width(x0, x, w);
  TORCH_CHECK(d > 0,
              "cin_layer kernels need bf16 x0 [B, m*D], x [B, H_in*D] and a "
              "contiguous weight [H_out, H_in, m] on one GPU with D in {16, "
              "32, 64}, 2 <= m <= ", CIN_MP, ", 1 <= H_in <= ", CIN_MAX_H,
              ", H_out % 16 == 0, 16 <= H_out <= ", CIN_MAX_H,
              ", unit column strides, row strides that are multiples of 8 "
              "elements and 16-byte aligned bases; got ", x0.sizes(), ", ",
              x.sizes(), ", ", w.sizes());
  return d;
}

void check_grad(const torch::Tensor& g, const torch::Tensor& x0,
                const torch::Tensor& w, int64_t d) {
  TORCH_CHECK(g.is_cuda() && g.device() == x0.device() && g.dim() == 2 &&
              g.size(0) == x0.size(0) && g.size(1) == w.size(0) * d,
              "grad_y must be [B, H_out*D] = [", x0.size(0), ", ",
              w.size(0) * d, "] on x0's GPU");
  TORCH_CHECK(rows_vector_ok(g),
              "grad_y must be bf16 with unit column stride, a row stride "
              "that is a multiple of 8 elements and no less than H_out*D, "
              "and a 16-byte aligned base");
}

int64_t block_cap(int64_t max_blocks) {
  TORCH_CHECK(max_blocks >= 0, "max_blocks must be >= 0 (0: the normal cap)");
  return max_blocks > 0 ? max_blocks : MIYARN_MAX_BLOCKS;
}

const unsigned short* cptr(const torch::Tensor& t) {
  return reinterpret_cast<const unsigned short*>(t.data_ptr());
}

unsigned short* mptr(torch::Tensor& t) {
  return reinterpret_cast<unsigned short*>(t.data_ptr());
}

// A packed copy of W (see cin_pack_kernel); hpad is used when transposed.
torch::Tensor pack_weight(const torch::Tensor& w, bool transposed, int hpad,
                          hipStream_t stream) {
  const int H_out = w.size(0), H_in = w.size(1), m = w.size(2);
  auto out = torch::empty(
      {(int64_t)H_in * CIN_MP * (transposed ? hpad : H_out)}, w.options());
  hipLaunchKernelGGL(cin_pack_kernel, dim3(miyarn_grid(out.numel())),
                     dim3(MIYARN_BLOCK), 0, stream, cptr(w), mptr(out), m,
                     H_in, H_out, hpad, transposed);
  return out;
}

}  // namespace

// True when cin_layer_fwd / _bwd_data / _bwd_weight take these operands.
bool cin_layer_ok(torch::Tensor x0, torch::Tensor x, torch::Tensor weight) {
  return cin_width(x0, x, weight) > 0;
}

// True when the backward kernels read this grad_y in place.
bool cin_layer_rows_ok(torch::Tensor grad_y) {
  return rows_vector_ok(grad_y);
}

torch::Tensor cin_layer_fwd(torch::Tensor x0, torch::Tensor x,
                            torch::Tensor weight, int64_t max_blocks) {
  const int64_t d = checked_width(x0, x, weight);
  const int64_t B = x0.size(0), H_out = weight.size(0);
  const int64_t cap = block_cap(max_blocks);
  auto y = torch::empty({B, H_out * d}, x0.options());
  if (B == 0) return y;
  auto stream = c10::hip::getCurrentHIPStream().stream();
  auto wp = pack_weight(weight, false, 0, stream);
  const int64_t items = B * (d / 16);
  constexpr int TRIP = CIN_WAVES * CIN_MT;
  const int grid = (int)std::min<int64_t>((items + TRIP - 1) / TRIP, cap);
  hipLaunchKernelGGL(cin_fwd_kernel, dim3(grid), dim3(MIYARN_BLOCK), 0,
                     stream, cptr(x0), cptr(x), cptr(wp), mptr(y), items,
                     (int)weight.size(2), (int)weight.size(1), (int)H_out,
                     (int)d, row_ld(x0), row_ld(x));
  return y;
}

// (dx [B, H_in*D], dx0 [B, m*D]), contiguous bf16.
std::vector<torch::Tensor> cin_layer_bwd_data(torch::Tensor grad_y,
                                              torch::Tensor x0,
                                              torch::Tensor x,
                                              torch::Tensor weight,
                                              int64_t max_blocks) {
  const int64_t d = checked_width(x0, x, weight);
  check_grad(grad_y, x0, weight, d);
  const int64_t B = x0.size(0);
  const int H_out = weight.size(0), H_in = weight.size(1), m = weight.size(2);
  const int64_t cap = block_cap(max_blocks);
  auto dx = torch::empty({B, H_in * d}, x0.options());
  auto dx0 = torch::empty({B, m * d}, x0.options());
  if (B == 0) return {dx, dx0};
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const int hpad = (H_out + 31) / 32 * 32;
  auto wt = pack_weight(weight, true, hpad, stream);
  const int64_t items = B * (d / 16);
  auto launch = [&](auto kernel, int ks, int mt) {
    const int ic = 16 / ks, trip = CIN_WAVES * mt;
    const size_t lds =
        (size_t)(ic * CIN_MP * (hpad + 8) + trip * ic * 16) * 2;
    const int grid = (int)std::min<int64_t>((items + trip - 1) / trip, cap);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(MIYARN_BLOCK), lds, stream,
                       cptr(grad_y), cptr(x0), cptr(x), cptr(wt), mptr(dx),
                       mptr(dx0), items, m, H_in, H_out, (int)d,
                       row_ld(grad_y), row_ld(x0), row_ld(x));
  };
  if (hpad <= 128) launch(cin_bwd_data_kernel<4, 4>, 4, 4);
  else launch(cin_bwd_data_kernel<8, 2>, 8, 2);
  return {dx, dx0};
}

// dW [H_out, H_in, m] bf16; max_blocks also caps the batch splits.
torch::Tensor cin_layer_bwd_weight(torch::Tensor grad_y, torch::Tensor x0,
                                   torch::Tensor x, torch::Tensor weight,
                                   int64_t max_blocks) {
  const int64_t d = checked_width(x0, x, weight);
  check_grad(grad_y, x0, weight, d);
  const int64_t B = x0.size(0);
  const int H_out = weight.size(0), H_in = weight.size(1), m = weight.size(2);
  const int64_t cap = block_cap(max_blocks);
  if (B == 0) return torch::zeros_like(weight);
  auto dw = torch::empty_like(weight);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const int tiles = H_in * (m > 16 ? 2 : 1);
  constexpr int PER_BLOCK = CIN_WAVES * CIN_WG_NT;
  const int tile_blocks = (tiles + PER_BLOCK - 1) / PER_BLOCK;
  const int h_blocks = (H_out + 16 * CIN_NT - 1) / (16 * CIN_NT);
  const int64_t total_k = B * d, steps = (total_k + 31) / 32;
  // enough blocks for two per CU, no more splits than the cap or the steps
  int64_t want = std::max<int64_t>(1, 512 / (tile_blocks * h_blocks));
  want = std::min({want, (int64_t)CIN_MAX_SPLITS, cap, steps});
  const int64_t per = (steps + want - 1) / want;
  const int splits = (int)((steps + per - 1) / per);  // none is empty
  auto part = torch::empty({(int64_t)splits * H_out * H_in * CIN_MP},
                           weight.options().dtype(torch::kFloat32));
  hipLaunchKernelGGL(cin_bwd_weight_kernel,
                     dim3(tile_blocks, splits, h_blocks), dim3(MIYARN_BLOCK),
                     0, stream, cptr(grad_y), cptr(x0), cptr(x),
                     part.data_ptr<float>(), total_k, per, m, H_in, H_out,
                     (int)d, row_ld(grad_y), row_ld(x0), row_ld(x));
  hipLaunchKernelGGL(cin_reduce_kernel,
                     dim3(miyarn_grid((int64_t)H_out * H_in * m)),
                     dim3(MIYARN_BLOCK), 0, stream, part.data_ptr<float>(),
                     mptr(dw), splits, m, H_out * H_in);
  return dw;
}
