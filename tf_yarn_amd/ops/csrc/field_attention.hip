// Multi-head self-attention over the per-example field embeddings (AutoInt,
// InterHAt) for MI355X, bf16, forward and backward.
//
// qkv is [B*N, 3*H*d]: row b*N + i is token i of example b as
// [q (H*d) | k (H*d) | v (H*d)], head h at columns h*d .. h*d + d - 1 of its
// third.  Per example b and head h, with Q, K, V the [N, d] slices and all
// sums in fp32:
//
//   s[i][j]  = scale * sum_c Q[i][c] * K[j][c]
//   m[i]     = max_j s[i][j]
//   p[i][j]  = exp(s[i][j] - m[i])
//   l[i]     = sum_j p[i][j]
//   Pb[i][j] = bf16(p[i][j] / l[i])              (the ONE attention matrix)
//   out[i][c] = bf16(sum_j Pb[i][j] * V[j][c])   (one rounding)
//
// Backward, with g = grad_out; it needs qkv and g only and recomputes Pb by
// the same code:
//
//   dV[j][c]  = bf16(sum_i Pb[i][j] * g[i][c])
//   dP[i][j]  = sum_c g[i][c] * V[j][c]
//   delta[i]  = sum_j Pb[i][j] * dP[i][j]
//   dSb[i][j] = bf16(scale * Pb[i][j] * (dP[i][j] - delta[i]))
//   dQ[i][c]  = bf16(sum_j dSb[i][j] * K[j][c])
//   dK[j][c]  = bf16(sum_i dSb[i][j] * Q[i][c])
//
// dS and delta take the ROUNDED Pb, the value the dV product sees.
//
// Both kernels give ONE WAVE ONE (example, head) per trip: a block is four
// waves with private LDS and the blocks grid-stride over groups of four
// items (every block makes whole trips, so its barriers are uniform).  One
// v_mfma_f32_32x32x16_bf16 tile holds a whole N x N matrix, N <= 32.
//
//  * Operand fragments: lane l loads 16 B of row l%32 of Q, K, V or g per
//    16-wide chunk of d, columns 8*(l/32) + 0..7: both the A[i][k] and the
//    B[k][n] fragment of that matrix (rows >= N are not loaded and zero).
//  * Scores as S^T = mfma(K, Q): register r of lane l holds key
//    8*(r/4) + 4*(l/32) + r%4 of query l%32, so a lane has 16 of its query's
//    32 scores and lane l^32 the other 16: max and sum are 16 in-register
//    operations and one exchange; m, 1/l (and delta) are per-lane scalars.
//    Keys >= N are set to -inf before the max.  A query column >= N computes
//    on a zero row (finite scores) and stores nothing.
//  * Pb stays in registers and is the B operand of the second product.  The
//    contraction index of an MFMA is a dummy: in chunk c of 16 keys the lane
//    of half h = l/32 holds keys {16c + 4h + 0..3, 16c + 8 + 4h + 0..3}, and
//    the A operand supplies V[j][col] for the same j: two groups of four
//    consecutive rows at one column, which is what ds_read_b64_tr_b16
//    delivers from a row-major [32][d] LDS image (lane 4q+p of a 16-lane
//    group points at row r0 + q, columns 4p..4p+3, and lane i receives
//    column i).  With V^T first the accumulator gives a lane four
//    CONSECUTIVE output columns of one token per register group: 8 B stores.
//    The image is written from the fragment registers, rows >= N as zeros.
//  * Backward: each tile in both orientations by swapping MFMA operands,
//    S^T = mfma(K, Q), S = mfma(Q, K), dP^T = mfma(V, g), dP = mfma(g, V),
//    from the same fragment registers.  The query-per-lane orientation gives
//    m, 1/l, delta, Pb^T and dSb^T and feeds dQ (contraction over keys); it
//    parks m, 1/l and delta (3 x 32 floats) in the wave's LDS.  The
//    key-per-lane orientation reads them back and forms the identical Pb and
//    dSb through the same two functions (prob_bits, ds_bits); it feeds dV
//    and dK (contractions over queries).  The contraction-strided operands,
//    K for dQ, g for dV, Q for dK, come from row-major LDS images through
//    the transposed read, as V does in the forward.
//    A dead query row i >= N adds exactly zero to dK and dV: its g row is
//    zero, so dP[i][.] = 0 and delta[i] = 0, dSb[i][j] =
//    bf16(scale * Pb * (0 - 0)) = 0, and its Pb[i][j] (finite: the row of Q
//    is zero, the scores are zero) multiplies g[i][c] = 0.
//
// P, dP and dS never reach global memory; there is no workspace, no atomic.
// N > 32, fp32, masks other than j >= N and dropout are not built.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include "mfma_tile.h"
#include <limits>
#include <vector>

namespace {

typedef __attribute__((ext_vector_type(16))) float mfma_f32x16;
typedef __attribute__((ext_vector_type(4))) __bf16 mfma_bf16x4;
#define FA_LDS_AS __attribute__((address_space(3)))
// the fp32 softmax arithmetic stays scalar instructions
#define FA_KERNEL __attribute__((target("no-packed-fp32-ops")))

constexpr int FA_WAVES = MIYARN_BLOCK / 64;
constexpr int FA_MAX_N = 32;
constexpr int FA_MAX_HD = 256;
constexpr int FA_STAT_BYTES = 3 * 32 * 4;  // m, 1/l, delta per query
constexpr float FA_LOG2E = 1.4426950408889634f;

__device__ __forceinline__ mfma_bf16x8 as_mfma(bf16x8 v) {
  return __builtin_bit_cast(mfma_bf16x8, v);
}

// __syncthreads(), spelled out: under FA_KERNEL's target attribute only
// forced-inline helpers are inlined, and the barrier should not be a call.
__device__ __forceinline__ void block_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ mfma_bf16x4 tr_read(const unsigned char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((FA_LDS_AS mfma_bf16x4*)p);
}

// The value of the lane 32 away.
__device__ __forceinline__ float half_swap(float x, int lane) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_ds_bpermute((lane ^ 32) << 2,
                                          __builtin_bit_cast(int, x)));
}

// Pb and dSb, for both orientations of the backward and for the forward.
__device__ __forceinline__ unsigned short prob_bits(float s, float m,
                                                    float inv) {
  return f32_to_bf16(__builtin_amdgcn_exp2f((s - m) * FA_LOG2E) * inv);
}

__device__ __forceinline__ unsigned short ds_bits(float scale,
                                                  unsigned short pb, float dp,
                                                  float delta) {
  return f32_to_bf16(scale * bf16_to_f32(pb) * (dp - delta));
}

// The key (query) that accumulator register r of a lane in half hh holds.
__device__ __forceinline__ int acc_row(int r, int hh) {
  return 8 * (r >> 2) + 4 * hh + (r & 3);
}

// m and 1/l of one query whose 32 masked scores are s[] here and in lane^32.
__device__ __forceinline__ void row_stats(const float (&s)[16], int lane,
                                          float& m, float& inv) {
  m = s[0];
#pragma unroll
  for (int r = 1; r < 16; ++r) m = __builtin_fmaxf(m, s[r]);
  m = __builtin_fmaxf(m, half_swap(m, lane));
  float l = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r)
    l += __builtin_amdgcn_exp2f((s[r] - m) * FA_LOG2E);
  l += half_swap(l, lane);
  inv = __builtin_amdgcn_rcpf(l);
}

// Byte offsets of a lane's transposed reads into a row-major [32][D] image:
// at[ct][cc][half] is the 4-row block 16*cc + 8*half + 4*(l/32) of the
// 16-column block 32*ct + 16*((l/16)%2).  At D = 16 the second column block
// wraps onto the first (its accumulator rows are never stored).
template <int D, int CT>
__device__ __forceinline__ void tr_offsets(int lane, int (&at)[CT][2][2]) {
  const int li = lane & 15, odd = (lane >> 4) & 1, hh = lane >> 5;
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int cc = 0; cc < 2; ++cc)
#pragma unroll
      for (int half = 0; half < 2; ++half)
        at[ct][cc][half] =
            ((16 * cc + 8 * half + 4 * hh + (li >> 2)) * D +
             (32 * ct + 16 * odd) % D + 4 * (li & 3)) * 2;
}

// out^T tile ct = image^T (32 columns) @ w, w[r] the lane's 16 contraction
// weights in accumulator order (see the head of the file).
template <int CT>
__device__ __forceinline__ mfma_f32x16 tr_product(const unsigned char* img,
                                                  const int (&at)[CT][2][2],
                                                  int ct,
                                                  const unsigned short (&w)[16]) {
  mfma_f32x16 o;
#pragma unroll
  for (int r = 0; r < 16; ++r) o[r] = 0.f;
#pragma unroll
  for (int cc = 0; cc < 2; ++cc) {
    const mfma_bf16x8 a = __builtin_shufflevector(
        tr_read(img + at[ct][cc][0]), tr_read(img + at[ct][cc][1]), 0, 1, 2,
        3, 4, 5, 6, 7);
    bf16x8 b;
#pragma unroll
    for (int e = 0; e < 8; ++e) b[e] = w[8 * cc + e];
    o = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, as_mfma(b), o, 0, 0, 0);
  }
  return o;
}

// The lane's part of tile ct: columns 32*ct + 8*g + 4*(l/32) + 0..3 of the
// token's D-wide slice at dst, 8 B per register group g.  `ok` masks the
// stores alone: the products before them need the whole wave.
template <int D>
__device__ __forceinline__ void store_tile(unsigned short* dst, bool ok,
                                           int ct, int hh,
                                           const mfma_f32x16& o) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int col = 32 * ct + 8 * g + 4 * hh;
    if (col >= D || !ok) continue;
    bf16x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = f32_to_bf16(o[4 * g + e]);
    *reinterpret_cast<bf16x4*>(dst + col) = v;
  }
}

template <int D>
__global__ FA_KERNEL __launch_bounds__(MIYARN_BLOCK) void
field_attention_fwd_kernel(const unsigned short* __restrict__ qkv,
                           unsigned short* __restrict__ out, int64_t items,
                           int N, int H, int64_t ld, float scale) {
  constexpr int KC = D / 16;         // 16-wide chunks of the head dimension
  constexpr int CT = (D + 31) / 32;  // 32-column tiles of the output
  __shared__ __attribute__((aligned(16))) unsigned char
      v_all[FA_WAVES][32 * D * 2];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  unsigned char* v_img = v_all[wave];
  const int row = lane & 31;  // the operand row; the query of S^T's column
  const int hh = lane >> 5;
  const int HD = H * D;
  int v_at[CT][2][2];
  tr_offsets<D, CT>(lane, v_at);
  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

  for (int64_t base = (int64_t)blockIdx.x * FA_WAVES; base < items;
       base += (int64_t)gridDim.x * FA_WAVES) {
    const int64_t item = base + wave;
    const bool live = item < items;
    const int64_t b = item / H;
    const int h = (int)(item - b * H);
    unsigned short pb[16];
    if (live) {
      const unsigned short* p = qkv + (b * N + row) * ld + h * D + hh * 8;
      mfma_f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
      for (int c = 0; c < KC; ++c) {
        bf16x8 q = zero8, k = zero8, v = zero8;
        if (row < N) {
          q = *reinterpret_cast<const bf16x8*>(p + 16 * c);
          k = *reinterpret_cast<const bf16x8*>(p + HD + 16 * c);
          v = *reinterpret_cast<const bf16x8*>(p + 2 * HD + 16 * c);
        }
        *reinterpret_cast<bf16x8*>(v_img + (row * D + 16 * c + 8 * hh) * 2) =
            v;
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_mfma(k), as_mfma(q),
                                                      acc, 0, 0, 0);
      }
      float s[16], m, inv;
#pragma unroll
      for (int r = 0; r < 16; ++r)
        s[r] = acc_row(r, hh) < N ? scale * acc[r]
                                  : -std::numeric_limits<float>::infinity();
      row_stats(s, lane, m, inv);
#pragma unroll
      for (int r = 0; r < 16; ++r) pb[r] = prob_bits(s[r], m, inv);
    }
    block_sync();
    if (live) {
      unsigned short* dst = out + (b * N + row) * HD + h * D;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
        store_tile<D>(dst, row < N, ct, hh,
                      tr_product<CT>(v_img, v_at, ct, pb));
    }
    block_sync();  // the image is rewritten next trip
  }
}

template <int D>
__global__ FA_KERNEL __launch_bounds__(MIYARN_BLOCK) void
field_attention_bwd_kernel(const unsigned short* __restrict__ qkv,
                           const unsigned short* __restrict__ g,
                           unsigned short* __restrict__ dqkv, int64_t items,
                           int N, int H, int64_t ld, int64_t g_ld,
                           float scale) {
  constexpr int KC = D / 16;
  constexpr int CT = (D + 31) / 32;
  constexpr int IMG = 32 * D * 2;
  extern __shared__ __attribute__((aligned(16))) unsigned char fa_lds[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  unsigned char* q_img = fa_lds + wave * (3 * IMG + FA_STAT_BYTES);
  unsigned char* k_img = q_img + IMG;
  unsigned char* g_img = k_img + IMG;
  float* stat = reinterpret_cast<float*>(g_img + IMG);
  const int row = lane & 31;
  const int hh = lane >> 5;
  const int HD = H * D;
  int at[CT][2][2];
  tr_offsets<D, CT>(lane, at);
  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  const float ninf = -std::numeric_limits<float>::infinity();

  for (int64_t base = (int64_t)blockIdx.x * FA_WAVES; base < items;
       base += (int64_t)gridDim.x * FA_WAVES) {
    const int64_t item = base + wave;
    const bool live = item < items;
    const int64_t b = item / H;
    const int h = (int)(item - b * H);
    unsigned short* drow = dqkv + (b * N + row) * (3 * (int64_t)HD) + h * D;
    bf16x8 qf[KC], kf[KC], vf[KC], gf[KC];
    unsigned short ds[16];
    if (live) {
      const unsigned short* p = qkv + (b * N + row) * ld + h * D + hh * 8;
      const unsigned short* pg = g + (b * N + row) * g_ld + h * D + hh * 8;
#pragma unroll
      for (int c = 0; c < KC; ++c) {
        qf[c] = kf[c] = vf[c] = gf[c] = zero8;
        if (row < N) {
          qf[c] = *reinterpret_cast<const bf16x8*>(p + 16 * c);
          kf[c] = *reinterpret_cast<const bf16x8*>(p + HD + 16 * c);
          vf[c] = *reinterpret_cast<const bf16x8*>(p + 2 * HD + 16 * c);
          gf[c] = *reinterpret_cast<const bf16x8*>(pg + 16 * c);
        }
        const int o = (row * D + 16 * c + 8 * hh) * 2;
        *reinterpret_cast<bf16x8*>(q_img + o) = qf[c];
        *reinterpret_cast<bf16x8*>(k_img + o) = kf[c];
        *reinterpret_cast<bf16x8*>(g_img + o) = gf[c];
      }
      // query per lane: S^T and dP^T, keys down the registers
      mfma_f32x16 st, dpt;
#pragma unroll
      for (int r = 0; r < 16; ++r) st[r] = dpt[r] = 0.f;
#pragma unroll
      for (int c = 0; c < KC; ++c) {
        st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            as_mfma(kf[c]), as_mfma(qf[c]), st, 0, 0, 0);
        dpt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            as_mfma(vf[c]), as_mfma(gf[c]), dpt, 0, 0, 0);
      }
      float s[16], m, inv;
#pragma unroll
      for (int r = 0; r < 16; ++r)
        s[r] = acc_row(r, hh) < N ? scale * st[r] : ninf;
      row_stats(s, lane, m, inv);
      unsigned short pb[16];
      float delta = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        pb[r] = prob_bits(s[r], m, inv);
        delta += bf16_to_f32(pb[r]) * dpt[r];
      }
      delta += half_swap(delta, lane);
#pragma unroll
      for (int r = 0; r < 16; ++r) ds[r] = ds_bits(scale, pb[r], dpt[r], delta);
      if (hh == 0) {
        stat[row] = m;
        stat[32 + row] = inv;
        stat[64 + row] = delta;
      }
    }
    block_sync();
    if (live) {
      // dQ^T = K^T dSb^T
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
        store_tile<D>(drow, row < N, ct, hh,
                      tr_product<CT>(k_img, at, ct, ds));
      // key per lane: S and dP, queries down the registers
      mfma_f32x16 sm, dp;
#pragma unroll
      for (int r = 0; r < 16; ++r) sm[r] = dp[r] = 0.f;
#pragma unroll
      for (int c = 0; c < KC; ++c) {
        sm = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            as_mfma(qf[c]), as_mfma(kf[c]), sm, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            as_mfma(gf[c]), as_mfma(vf[c]), dp, 0, 0, 0);
      }
      unsigned short pb[16];
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int i0 = 8 * g4 + 4 * hh;  // acc_row(4 * g4, hh)
        const f32x4 m4 = *reinterpret_cast<const f32x4*>(stat + i0);
        const f32x4 inv4 = *reinterpret_cast<const f32x4*>(stat + 32 + i0);
        const f32x4 del4 = *reinterpret_cast<const f32x4*>(stat + 64 + i0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * g4 + e;
          const float sc = row < N ? scale * sm[r] : ninf;
          pb[r] = prob_bits(sc, m4[e], inv4[e]);
          ds[r] = ds_bits(scale, pb[r], dp[r], del4[e]);
        }
      }
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        // dV^T = g^T Pb and dK^T = Q^T dSb
        store_tile<D>(drow + 2 * HD, row < N, ct, hh,
                      tr_product<CT>(g_img, at, ct, pb));
        store_tile<D>(drow + HD, row < N, ct, hh,
                      tr_product<CT>(q_img, at, ct, ds));
      }
    }
    block_sync();  // the images and the statistics are rewritten next trip
  }
}

// [rows, cols] bf16 with unit column stride, rows a multiple of 8 elements
// and at least their own width apart (no expanded or overlapping rows) and
// a 16 B aligned base: what the 16 B loads need.
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

// The head dimension the kernels take for these operands, or 0.
int64_t head_dim(const torch::Tensor& qkv, int64_t n_fields, int64_t n_heads) {
  if (!rows_vector_ok(qkv) || n_fields < 1 || n_fields > FA_MAX_N ||
      n_heads < 1 || qkv.size(0) % n_fields != 0 ||
      qkv.size(1) % (3 * n_heads) != 0)
    return 0;
  const int64_t d = qkv.size(1) / (3 * n_heads);
  return (d == 16 || d == 32 || d == 64) && n_heads * d <= FA_MAX_HD ? d : 0;
}

int fa_grid(int64_t items, int64_t max_blocks) {
  TORCH_CHECK(max_blocks >= 0, "max_blocks must be >= 0 (0: the normal cap)");
  return miyarn_grid_cap(items * 64, max_blocks > 0 ? max_blocks
                                                    : MIYARN_MAX_BLOCKS);
}

int64_t checked_head_dim(const torch::Tensor& qkv, int64_t n_fields,
                         int64_t n_heads) {
  const int64_t d = head_dim(qkv, n_fields, n_heads);
  TORCH_CHECK(d > 0,
              "field_attention kernels need bf16 qkv [B*N, 3*H*d] on the GPU "
              "with 1 <= N <= ", FA_MAX_N, ", d in {16, 32, 64}, H*d <= ",
              FA_MAX_HD, ", unit column stride, a row stride that is a "
              "multiple of 8 elements and a 16-byte aligned base; got ",
              qkv.sizes(), ", N = ", n_fields, ", H = ", n_heads);
  return d;
}

}  // namespace

// True when field_attention_fwd / _bwd take these operands.
bool field_attention_ok(torch::Tensor qkv, int64_t n_fields,
                        int64_t n_heads) {
  return head_dim(qkv, n_fields, n_heads) > 0;
}

// True when field_attention_bwd reads this grad_out in place: the layout
// test of its TORCH_CHECK, for the caller that would rather copy than raise.
bool field_attention_rows_ok(torch::Tensor grad_out) {
  return rows_vector_ok(grad_out);
}

torch::Tensor field_attention_fwd(torch::Tensor qkv, int64_t n_fields,
                                  int64_t n_heads, double scale,
                                  int64_t max_blocks) {
  const int64_t d = checked_head_dim(qkv, n_fields, n_heads);
  const int64_t rows = qkv.size(0), HD = n_heads * d;
  const int64_t items = rows / n_fields * n_heads;
  auto out = torch::empty({rows, HD}, qkv.options());
  const int grid = fa_grid(items, max_blocks);
  if (items == 0) return out;
  auto stream = c10::hip::getCurrentHIPStream().stream();
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(
        kernel, dim3(grid), dim3(MIYARN_BLOCK), 0, stream,
        reinterpret_cast<const unsigned short*>(qkv.data_ptr()),
        reinterpret_cast<unsigned short*>(out.data_ptr()), items,
        (int)n_fields, (int)n_heads, row_ld(qkv), (float)scale);
  };
  if (d == 16) launch(field_attention_fwd_kernel<16>);
  else if (d == 32) launch(field_attention_fwd_kernel<32>);
  else launch(field_attention_fwd_kernel<64>);
  return out;
}

// dqkv [B*N, 3*H*d], contiguous bf16, in qkv's packed layout.
torch::Tensor field_attention_bwd(torch::Tensor grad_out, torch::Tensor qkv,
                                  int64_t n_fields, int64_t n_heads,
                                  double scale, int64_t max_blocks) {
  const int64_t d = checked_head_dim(qkv, n_fields, n_heads);
  const int64_t rows = qkv.size(0), HD = n_heads * d;
  const int64_t items = rows / n_fields * n_heads;
  TORCH_CHECK(grad_out.is_cuda() && grad_out.device() == qkv.device() &&
              grad_out.dim() == 2 && grad_out.size(0) == rows &&
              grad_out.size(1) == HD,
              "grad_out must be [B*N, H*d] = [", rows, ", ", HD,
              "] on qkv's GPU");
  TORCH_CHECK(rows_vector_ok(grad_out),
              "grad_out must be bf16 with unit column stride, a row stride "
              "that is a multiple of 8 elements and no less than H*d, and a "
              "16-byte aligned base");
  auto dqkv = torch::empty({rows, 3 * HD}, qkv.options());
  const int grid = fa_grid(items, max_blocks);
  if (items == 0) return dqkv;
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const size_t lds = (size_t)FA_WAVES * (3 * 32 * d * 2 + FA_STAT_BYTES);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(
        kernel, dim3(grid), dim3(MIYARN_BLOCK), lds, stream,
        reinterpret_cast<const unsigned short*>(qkv.data_ptr()),
        reinterpret_cast<const unsigned short*>(grad_out.data_ptr()),
        reinterpret_cast<unsigned short*>(dqkv.data_ptr()), items,
        (int)n_fields, (int)n_heads, row_ld(qkv), row_ld(grad_out),
        (float)scale);
  };
  if (d == 16) launch(field_attention_bwd_kernel<16>);
  else if (d == 32) launch(field_attention_bwd_kernel<32>);
  else launch(field_attention_bwd_kernel<64>);
  return dqkv;
}
