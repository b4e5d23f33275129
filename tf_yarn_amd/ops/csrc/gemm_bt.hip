// Forward GEMM C[M, N] = A[M, K] @ B[N, K]^T with optional fused
// bias+ReLU epilogue — the nn.Linear forward shape (x @ W.t()).
//
// Both operands are stored K-MAJOR (row-major with K innermost), which is
// exactly what the mfma_f32_16x16x32_bf16 fragments want (8 consecutive k
// per lane): staging into LDS is a LINEAR copy, no transpose — only the
// fragment reads/writes use the XOR swizzle (mfma_tile.h, lds_off_linear;
// the 256x256 tile / 8-wave / 4x8-fragment geometry of wgrad's TILE=256).
// Tile map, staging and k-step are mfma_tile.h's.
// K is tail-masked (K % 64 != 0 OK, K % 16 == 0 required); B rows are
// masked so N % 256 != 0 works (the 432-wide dgrad shape).
//
// The bias+ReLU epilogue writes bf16 C directly, eliminating the separate
// bias_relu kernel AND the pre-activation round trip through HBM.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include "mfma_tile.h"

namespace {

#define G_BM 256  // rows of A per tile
#define G_BN 256  // rows of B (= output cols) per tile
#define G_BK 64

template <bool RELU>
__global__ __launch_bounds__(512)
void gemm_bt_kernel(const unsigned short* __restrict__ A,
                    const unsigned short* __restrict__ B,
                    const unsigned short* __restrict__ bias,  // may be null
                    unsigned short* __restrict__ C,
                    int64_t M, int N, int K) {
  const int tiles_n = (N + G_BN - 1) / G_BN;
  const int tiles_m = static_cast<int>(M / G_BM);
  int tile_m, tile_n;
  xcd_tile_map(tiles_m, tiles_n, tile_m, tile_n);  // shares the A rows
  const int64_t m0 = (int64_t)tile_m * G_BM;
  const int n0 = tile_n * G_BN;

  __shared__ __attribute__((aligned(16))) unsigned char lds_raw[2 * 256 * 128];
  unsigned char* aT = lds_raw;              // [256 m][64 k] swizzled
  unsigned char* bT = lds_raw + 256 * 128;  // [256 n][64 k]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = (wave >> 1) * 64;   // 4 M-quadrants of 64
  const int wn = (wave & 1) * 128;   // 2 N-halves of 128

  // both operands take mfma_tile.h's K-major staging
  const int st_r = tid >> 1;
  const int st_k = (tid & 1) * 32;
  const bool b_row_ok = (n0 + st_r) < N;  // B rows masked for ragged N

  mfma_f32x4 acc[4][8];
  zero_acc(acc);

  bf16x8 ra[4], rb[4];

  auto load_step = [&](int k0) {
    stage_kmajor_load(ra, A + (m0 + st_r) * (int64_t)K + k0 + st_k, true,
                      k0 + st_k, K);
    stage_kmajor_load(rb, B + (int64_t)(n0 + st_r) * K + k0 + st_k, b_row_ok,
                      k0 + st_k, K);
  };

  load_step(0);
  for (int k0 = 0; k0 < K; k0 += G_BK) {
    stage_kmajor_write(aT, ra, st_r, st_k);
    stage_kmajor_write(bT, rb, st_r, st_k);
    __syncthreads();
    if (k0 + G_BK < K) load_step(k0 + G_BK);  // in flight under MFMA
    mfma_kstep<4, 8, lds_off_linear, lds_off_linear, false>(acc, aT, bT, wm,
                                                            wn, lane);
    __syncthreads();
  }

  // epilogue: bf16 C with optional bias+ReLU; A-fragments index M (rows),
  // B-fragments index N (cols): D col = lane&15 -> N, row -> M.
  int f_col, f_row4;
  frag_pos(lane, f_col, f_row4);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int col = n0 + wn + j * 16 + f_col;
      if (col >= N) continue;
      const float bv = bias ? bf16_to_f32(bias[col]) : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = m0 + wm + i * 16 + f_row4 + r;
        float v = acc[i][j][r] + bv;
        if (RELU) v = v > 0.f ? v : 0.f;
        C[row * N + col] = f32_to_bf16(v);
      }
    }
}

}  // namespace

torch::Tensor gemm_bt(torch::Tensor a, torch::Tensor b,
                      c10::optional<torch::Tensor> bias, bool relu) {
  TORCH_CHECK(a.is_cuda() && a.is_contiguous() && a.dim() == 2 &&
              a.scalar_type() == torch::kBFloat16,
              "a must be [M, K] bf16 contiguous");
  TORCH_CHECK(b.is_cuda() && b.is_contiguous() && b.dim() == 2 &&
              b.scalar_type() == torch::kBFloat16,
              "b must be [N, K] bf16 contiguous");
  const int64_t M = a.size(0);
  const int K = static_cast<int>(a.size(1));
  const int N = static_cast<int>(b.size(0));
  TORCH_CHECK(b.size(1) == K, "K mismatch");
  TORCH_CHECK(M % G_BM == 0 && N % 16 == 0 && K % 16 == 0,
              "gemm_bt needs M % 256 == 0, N % 16 == 0, K % 16 == 0");
  const unsigned short* bias_ptr = nullptr;
  if (bias.has_value()) {
    TORCH_CHECK(bias->is_cuda() && bias->is_contiguous() &&
                bias->scalar_type() == torch::kBFloat16 &&
                bias->numel() == N, "bias must be [N] bf16");
    bias_ptr = reinterpret_cast<const unsigned short*>(bias->data_ptr());
  }
  auto c = torch::empty({M, (int64_t)N},
                        a.options().dtype(torch::kBFloat16));
  auto stream = c10::hip::getCurrentHIPStream().stream();
  dim3 grid((M / G_BM) * ((N + G_BN - 1) / G_BN));
  auto* kern = relu ? gemm_bt_kernel<true> : gemm_bt_kernel<false>;
  hipLaunchKernelGGL(kern, grid, dim3(512), 0, stream,
                     reinterpret_cast<const unsigned short*>(a.data_ptr()),
                     reinterpret_cast<const unsigned short*>(b.data_ptr()),
                     bias_ptr,
                     reinterpret_cast<unsigned short*>(c.data_ptr()),
                     M, N, K);
  return c;
}
