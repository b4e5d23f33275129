// Pairwise dot feature interaction (DLRM's "dot" interaction without
// self-interaction) for MI355X, bf16, forward and backward.
//
// Per example b, T[b] is the [N, D] matrix whose row 0 is dense_vec[b] and
// whose row 1 + f is emb[b, f*D : (f+1)*D]; N = F + 1, P = N*(N-1)/2 and
// W = D + P rounded up to a multiple of 16:
//
//   out[b, c]                 = dense_vec[b, c]                  c < D
//   out[b, D + i*(i-1)/2 + j] = sum_k T[b,i,k] * T[b,j,k]        j < i < N
//   out[b, D + P .. W-1]      = 0
//
// with fp32 products and sums and ONE rounding to bf16.  Backward, with
// g = grad_out and S[b] the symmetric [N, N] matrix S[i][j] = S[j][i] =
// g[b, D + i*(i-1)/2 + j], zero diagonal:
//
//   dT[b] = S[b] @ T[b]                       (fp32 accumulation)
//   d_dense_vec[b, c] = round(float(g[b, c]) + dT[b, 0, c])
//   d_emb[b, f*D + c] = round(dT[b, 1 + f, c])
//
// Both kernels give ONE WAVE ONE EXAMPLE per trip: a block is four waves
// with private LDS tiles and the blocks grid-stride over groups of four
// examples (every block makes whole trips, so its barriers are uniform).
//
//  * forward: for v_mfma_f32_32x32x16_bf16 lane l supplies
//    A[i = l%32][k = 8*(l/32) + 0..7] and B[k = 8*(l/32) + 0..7][n = l%32];
//    with B = T^T those are the same eight values, so the lane's one 16 B
//    global load of row l%32 (row 0 from dense_vec, rows >= N not loaded and
//    zero) is both operands and Z = mfma(a, a, Z) over the D/16 chunks of k
//    is the example's whole Gram matrix; the input never touches LDS.  The
//    accumulator holds Z[8*(r/4) + 4*(l/32) + r%4][l%32] in register r of
//    16.  The wave parks Z in its [32][32] fp32 tile and writes the W-wide
//    output row front to back, 16 B per lane: the pass-through columns
//    straight from dense_vec, then the packed triangle and the pad, eight
//    tile words per lane.  Which words is the same for every example: each
//    lane works out its (i, j) once, before the loop, and a pad column reads
//    a word of the tile that is always zero.
//  * backward: the wave copies the gradient row and the example's N rows of
//    T into LDS with coalesced 16 B loads, T as a [32 k][D] image whose
//    rows >= N were zeroed once.  dT^T = T^T @ S: the A fragment
//    A[c][k] = T[k][c] comes out of the image through ds_read_b64_tr_b16
//    (the map of mfma_tile.h's third image: lane 4q+p of a 16-lane group
//    reads row r0 + q, columns 4p..4p+3, and lane i receives column i), the
//    B fragment B[k][i] = S[k][i] is eight 2-byte reads of the gradient row
//    at packed(max, min) (the diagonal and rows or columns >= N read the
//    row's zero word), again the same places for every example.  Two
//    mfma_f32_16x16x32_bf16 per 16 columns of D, K = 32 being the padded N.
//    With T^T first the accumulator's four registers are four CONSECUTIVE
//    columns c of one row i, so a lane stores 8 B and the four lanes of a
//    row 32 B; at D = 16 a whole store instruction is 512 contiguous bytes.
//
// S is symmetric and so is Z: swapping row and column of either fragment
// map would go unnoticed, a wrong row SET would not
// (tests/test_dot_interaction_gpu.py compares bit for bit).
// N > 32 (a 2x2 tile of MFMAs per example), fp32 and self-interaction are
// not built.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include "mfma_tile.h"
#include <vector>

namespace {

typedef __attribute__((ext_vector_type(16))) float mfma_f32x16;
typedef __attribute__((ext_vector_type(4))) __bf16 mfma_bf16x4;
#define DI_LDS_AS __attribute__((address_space(3)))
// the few fp32 operations here stay scalar instructions
#define DI_KERNEL __attribute__((target("no-packed-fp32-ops")))

constexpr int DI_WAVES = MIYARN_BLOCK / 64;
constexpr int DI_MAX_N = 32;
constexpr int DI_MAX_D = 128;
constexpr int DI_MAX_W = DI_MAX_D + DI_MAX_N * (DI_MAX_N - 1) / 2;  // 624
// forward tile: Z[32][32] fp32 and, behind it, the word the pad reads
constexpr int DI_Z_ZERO = 32 * 32;
constexpr int DI_Z_WORDS = DI_Z_ZERO + 4;
// backward gradient row: W <= 624 bf16 and, behind them, eight zeros
constexpr int DI_G_ZERO = DI_MAX_W;
constexpr int DI_G_BYTES = (DI_MAX_W + 8) * 2;

static_assert(DI_MAX_W % 16 == 0 && DI_G_BYTES % 16 == 0, "16 B LDS vectors");

// Packed position q of the strictly lower triangle -> (i, j), j < i.
__device__ __forceinline__ void tri_ij(int q, int& i, int& j) {
  i = 1;
  while (i * (i + 1) / 2 <= q) ++i;
  j = q - i * (i - 1) / 2;
}

__device__ __forceinline__ mfma_bf16x8 as_mfma(bf16x8 v) {
  return __builtin_bit_cast(mfma_bf16x8, v);
}

// __syncthreads(), spelled out: under DI_KERNEL's target attribute only
// forced-inline helpers are inlined, and the barrier should not be a call.
__device__ __forceinline__ void block_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ mfma_bf16x4 tr_read(const unsigned char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((DI_LDS_AS mfma_bf16x4*)p);
}

__global__ DI_KERNEL __launch_bounds__(MIYARN_BLOCK) void
dot_interaction_fwd_kernel(const unsigned short* __restrict__ dense,
                           const unsigned short* __restrict__ emb,
                           unsigned short* __restrict__ out, int64_t B, int N,
                           int D, int W, int64_t dense_ld, int64_t emb_ld) {
  __shared__ float z_all[DI_WAVES][DI_Z_WORDS];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  float* z = z_all[wave];
  const int P = N * (N - 1) / 2;
  const int row = lane & 31;  // the operand row, and Z's column
  const int kh = lane >> 5;

  // The lane's output chunks (8 columns each; W <= 624 is at most 78, two
  // per lane) and the tile words of their triangle and pad columns.
  int src[2][8];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int q0 = (lane + 64 * s) * 8 - D;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      src[s][e] = DI_Z_ZERO;
      if (q0 >= 0 && q0 + e < P) {
        int i, j;
        tri_ij(q0 + e, i, j);
        src[s][e] = i * 32 + j;
      }
    }
  }
  if (lane < DI_Z_WORDS - DI_Z_ZERO) z[DI_Z_ZERO + lane] = 0.f;

  for (int64_t base = (int64_t)blockIdx.x * DI_WAVES; base < B;
       base += (int64_t)gridDim.x * DI_WAVES) {
    const int64_t b = base + wave;
    const bool live = b < B;
    const unsigned short* drow = dense + b * dense_ld;
    if (live) {
      const unsigned short* p =
          (row == 0 ? drow : emb + b * emb_ld + (row - 1) * D) + kh * 8;
      mfma_f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      for (int c = 0; c < D; c += 16) {
        bf16x8 a = {0, 0, 0, 0, 0, 0, 0, 0};
        if (row < N) a = *reinterpret_cast<const bf16x8*>(p + c);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_mfma(a), as_mfma(a),
                                                      acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r)
        z[(8 * (r >> 2) + 4 * kh + (r & 3)) * 32 + row] = acc[r];
    }
    block_sync();
    if (live) {
      unsigned short* orow = out + b * W;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int col = (lane + 64 * s) * 8;
        if (col >= W) continue;
        bf16x8 v;
        if (col < D) {
          v = *reinterpret_cast<const bf16x8*>(drow + col);
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = f32_to_bf16(z[src[s][e]]);
        }
        *reinterpret_cast<bf16x8*>(orow + col) = v;
      }
    }
    block_sync();  // the tile is parked again next trip
  }
}

__global__ DI_KERNEL __launch_bounds__(MIYARN_BLOCK) void
dot_interaction_bwd_kernel(const unsigned short* __restrict__ g,
                           const unsigned short* __restrict__ dense,
                           const unsigned short* __restrict__ emb,
                           unsigned short* __restrict__ d_dense,
                           unsigned short* __restrict__ d_emb, int64_t B,
                           int N, int D, int W, int64_t g_ld,
                           int64_t dense_ld, int64_t emb_ld) {
  extern __shared__ __attribute__((aligned(16))) unsigned char di_lds[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int t_bytes = 32 * D * 2;  // the [32 k][D] image of T
  unsigned char* t_img = di_lds + wave * (t_bytes + DI_G_BYTES);
  unsigned short* g_row = reinterpret_cast<unsigned short*>(t_img + t_bytes);
  const int dvec = D / 8;           // 16 B vectors per row of T
  const int t_vecs = N * dvec;      // ... per example
  const int g_vecs = W / 8;
  const int col = lane & 15;  // fragment column: dT's row i (mod 16)
  const int grp = lane >> 4;

  // rows >= N of the image and the gradient row's zero word: written once
  const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int t = t_vecs + lane; t < 32 * dvec; t += 64)
    *reinterpret_cast<bf16x8*>(t_img + t * 16) = zero8;
  if (lane == 0) *reinterpret_cast<bf16x8*>(g_row + DI_G_ZERO) = zero8;

  // B fragment of S for dT rows 16*nb + col: element j is S[k][i],
  // k = 8*grp + j, at these places of the gradient row
  int s_at[2][8];
#pragma unroll
  for (int nb = 0; nb < 2; ++nb) {
    const int i = 16 * nb + col;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = 8 * grp + j;
      const int hi = max(i, k), lo = min(i, k);
      s_at[nb][j] =
          (i != k && hi < N) ? D + hi * (hi - 1) / 2 + lo : DI_G_ZERO;
    }
  }
  // A fragment of T^T: two transposed reads, k-rows 8*grp + 4*h + q,
  // columns 4p..4p+3 of the 16-column block
  int t_at[2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
    t_at[h] = (8 * grp + 4 * h + (col >> 2)) * D * 2 + (col & 3) * 8;

  for (int64_t base = (int64_t)blockIdx.x * DI_WAVES; base < B;
       base += (int64_t)gridDim.x * DI_WAVES) {
    const int64_t b = base + wave;
    const bool live = b < B;
    if (live) {
      const unsigned short* grow = g + b * g_ld;
      const unsigned short* drow = dense + b * dense_ld;
      const unsigned short* erow = emb + b * emb_ld;
      bf16x8 gv[2] = {zero8, zero8};
#pragma unroll
      for (int s = 0; s < 2; ++s)
        if (lane + 64 * s < g_vecs)
          gv[s] = *reinterpret_cast<const bf16x8*>(grow + (lane + 64 * s) * 8);
      for (int t = lane; t < t_vecs; t += 64)
        *reinterpret_cast<bf16x8*>(t_img + t * 16) =
            *reinterpret_cast<const bf16x8*>(
                t < dvec ? drow + t * 8 : erow + (t - dvec) * 8);
#pragma unroll
      for (int s = 0; s < 2; ++s)
        if (lane + 64 * s < g_vecs)
          *reinterpret_cast<bf16x8*>(g_row + (lane + 64 * s) * 8) = gv[s];
    }
    block_sync();
    if (live) {
      mfma_bf16x8 s_frag[2];
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        bf16x8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = g_row[s_at[nb][j]];
        s_frag[nb] = as_mfma(v);
      }
      for (int cb = 0; cb < D; cb += 16) {
        const mfma_bf16x8 t_frag = __builtin_shufflevector(
            tr_read(t_img + t_at[0] + cb * 2),
            tr_read(t_img + t_at[1] + cb * 2), 0, 1, 2, 3,
            4, 5, 6, 7);
        const int c0 = cb + grp * 4;
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
          const int i = 16 * nb + col;
          const mfma_f32x4 acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              t_frag, s_frag[nb], mfma_f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
          if (i >= N) continue;
          bf16x4 v;
#pragma unroll
          for (int r = 0; r < 4; ++r)
            v[r] = f32_to_bf16(
                i == 0 ? acc[r] + bf16_to_f32(g_row[c0 + r]) : acc[r]);
          unsigned short* dst = i == 0 ? d_dense + b * D + c0
                                       : d_emb + b * (int64_t)(N - 1) * D +
                                             (i - 1) * D + c0;
          *reinterpret_cast<bf16x4*>(dst) = v;
        }
      }
    }
    block_sync();  // the image and the row are refilled next trip
  }
}

// [B, cols] bf16 with unit column stride, rows a multiple of 8 elements
// and at least their own width apart (no expanded or overlapping rows) and
// a 16 B aligned base: what the 16 B loads need.
bool rows_vector_ok(const torch::Tensor& t) {
  return t.dim() == 2 && t.scalar_type() == torch::kBFloat16 &&
         (t.size(1) <= 1 || t.stride(1) == 1) &&
         (t.size(0) <= 1 ||
          (t.stride(0) >= t.size(1) && t.stride(0) % 8 == 0)) &&
         miyarn_aligned(t.data_ptr(), 16);
}

int64_t row_ld(const torch::Tensor& t) {
  return t.size(0) > 1 ? t.stride(0) : t.size(1);
}

int di_grid(int64_t B, int64_t max_blocks) {
  TORCH_CHECK(max_blocks >= 0, "max_blocks must be >= 0 (0: the normal cap)");
  return miyarn_grid_cap(B * 64, max_blocks > 0 ? max_blocks
                                                : MIYARN_MAX_BLOCKS);
}

// The (n_features, dim) the kernels take.
bool shape_ok(int64_t n_features, int64_t dim) {
  return dim >= 16 && dim % 16 == 0 && dim <= DI_MAX_D && n_features >= 1 &&
         n_features + 1 <= DI_MAX_N;
}

int64_t out_width(int64_t n_features, int64_t dim) {
  const int64_t n = n_features + 1;
  return (dim + n * (n - 1) / 2 + 15) / 16 * 16;
}

void check_operands(const torch::Tensor& dense_vec, const torch::Tensor& emb) {
  TORCH_CHECK(dense_vec.is_cuda() && emb.is_cuda() &&
              dense_vec.device() == emb.device(),
              "dense_vec and emb must be on one GPU");
  TORCH_CHECK(dense_vec.scalar_type() == torch::kBFloat16 &&
              emb.scalar_type() == torch::kBFloat16,
              "dot_interaction kernels: bf16 only");
  TORCH_CHECK(dense_vec.dim() == 2 && emb.dim() == 2 &&
              dense_vec.size(0) == emb.size(0),
              "dense_vec must be [B, D] and emb [B, F*D]");
  const int64_t dim = dense_vec.size(1);
  TORCH_CHECK(dim > 0 && emb.size(1) % dim == 0,
              "emb.size(1) = ", emb.size(1), " is no multiple of D = ", dim);
  TORCH_CHECK(shape_ok(emb.size(1) / dim, dim),
              "dot_interaction kernels need D % 16 == 0, D <= ", DI_MAX_D,
              " and 2 <= N = F + 1 <= ", DI_MAX_N, ", got D = ", dim,
              ", F = ", emb.size(1) / dim);
  TORCH_CHECK(rows_vector_ok(dense_vec) && rows_vector_ok(emb),
              "dense_vec and emb need unit column stride, a row stride that "
              "is a multiple of 8 elements and a 16-byte aligned base");
}

}  // namespace

// True when dot_interaction_fwd / _bwd take these operands.
bool dot_interaction_ok(torch::Tensor dense_vec, torch::Tensor emb) {
  if (!(dense_vec.is_cuda() && emb.is_cuda() &&
        dense_vec.device() == emb.device() && rows_vector_ok(dense_vec) &&
        rows_vector_ok(emb) && dense_vec.size(0) == emb.size(0)))
    return false;
  const int64_t dim = dense_vec.size(1);
  return dim > 0 && emb.size(1) % dim == 0 &&
         shape_ok(emb.size(1) / dim, dim);
}

// True when dot_interaction_bwd reads this grad_out in place: the layout
// test of its TORCH_CHECK, for the caller that would rather copy than raise.
bool dot_interaction_grad_ok(torch::Tensor grad_out) {
  return grad_out.is_cuda() && rows_vector_ok(grad_out);
}

torch::Tensor dot_interaction_fwd(torch::Tensor dense_vec, torch::Tensor emb,
                                  int64_t max_blocks) {
  check_operands(dense_vec, emb);
  const int64_t B = dense_vec.size(0);
  const int D = (int)dense_vec.size(1);
  const int N = (int)(emb.size(1) / D) + 1;
  const int W = (int)out_width(N - 1, D);
  auto out = torch::empty({B, W}, dense_vec.options());
  const int grid = di_grid(B, max_blocks);
  if (B == 0) return out;
  auto stream = c10::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(
      dot_interaction_fwd_kernel, dim3(grid), dim3(MIYARN_BLOCK), 0, stream,
      reinterpret_cast<const unsigned short*>(dense_vec.data_ptr()),
      reinterpret_cast<const unsigned short*>(emb.data_ptr()),
      reinterpret_cast<unsigned short*>(out.data_ptr()), B, N, D, W,
      row_ld(dense_vec), row_ld(emb));
  return out;
}

// {d_dense_vec [B, D], d_emb [B, F*D]}, both contiguous bf16.
std::vector<torch::Tensor> dot_interaction_bwd(torch::Tensor grad_out,
                                               torch::Tensor dense_vec,
                                               torch::Tensor emb,
                                               int64_t max_blocks) {
  check_operands(dense_vec, emb);
  const int64_t B = dense_vec.size(0);
  const int D = (int)dense_vec.size(1);
  const int N = (int)(emb.size(1) / D) + 1;
  const int W = (int)out_width(N - 1, D);
  TORCH_CHECK(grad_out.is_cuda() && grad_out.device() == emb.device() &&
              grad_out.dim() == 2 && grad_out.size(0) == B &&
              grad_out.size(1) == W,
              "grad_out must be [B, W] = [", B, ", ", W, "] on emb's GPU");
  TORCH_CHECK(rows_vector_ok(grad_out),
              "grad_out must be bf16 with unit column stride, a row stride "
              "that is a multiple of 8 elements and no less than W, and a "
              "16-byte aligned base");
  auto d_dense = torch::empty({B, D}, dense_vec.options());
  auto d_emb = torch::empty({B, emb.size(1)}, emb.options());
  const int grid = di_grid(B, max_blocks);
  if (B == 0) return {d_dense, d_emb};
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const size_t lds = (size_t)DI_WAVES * (32 * D * 2 + DI_G_BYTES);
  hipLaunchKernelGGL(
      dot_interaction_bwd_kernel, dim3(grid), dim3(MIYARN_BLOCK), lds, stream,
      reinterpret_cast<const unsigned short*>(grad_out.data_ptr()),
      reinterpret_cast<const unsigned short*>(dense_vec.data_ptr()),
      reinterpret_cast<const unsigned short*>(emb.data_ptr()),
      reinterpret_cast<unsigned short*>(d_dense.data_ptr()),
      reinterpret_cast<unsigned short*>(d_emb.data_ptr()), B, N, D, W,
      row_ld(grad_out), row_ld(dense_vec), row_ld(emb));
  return {d_dense, d_emb};
}
