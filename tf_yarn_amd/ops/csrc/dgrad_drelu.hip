// Hidden-layer dgrad with the ReLU backward of the layer below and its
// bias gradient in the epilogue:
//
//   acc[m, n] = sum_k dz_next[m, k] * w[k, n]          fp32, MFMA
//   dz[m, n]  = y[m, n] > 0 ? bf16_rne(acc[m, n]) : 0
//   dbias[n]  = sum_m float(dz[m, n])                  of the rounded values
//
// which is bias_relu_bwd_db(dz_next @ w, y) without dx = dz_next @ w in
// memory.  hipBLASLt has no DReLU+bias-gradient epilogue, so this is the
// one GEMM of the step the library cannot fuse.
//
// Operands.  dz_next [M, K] is K-major and stages linearly (gemm_bt's A
// operand, lds_off_linear).  w [K, N] is the weight as stored: its rows
// are the reduction index and N is contiguous, the shape of wgrad_kernel's
// x operand, so it takes that staging: coalesced 16 B row loads, packed
// b64 transposed LDS writes under lds_off, columns masked at the ragged
// tile.  No W^T copy is made.
//
// The MFMA takes the w fragment FIRST: D's row index (four consecutive
// per lane) is then n and its column index (lane & 15) is m, so a lane
// holds four adjacent columns of one output row and parks them as one
// packed b64.
//
// Epilogue.  After the k-loop's last barrier the operand buffers are free.
// The tile goes through them in two column halves: the waves that own the
// half round their accumulators to bf16 and park them row-major (16 B
// chunks XOR-swizzled by row, so the parking writes and the row reads both
// spread over the banks), then ALL threads walk the half the way
// bias_relu_bwd_dbpart8_body walks rows: a thread owns one oct of columns,
// takes y as bf16x8 from memory and its C oct from LDS, masks, stores
// bf16x8 and keeps eight fp32 column sums.  The y loads of both halves are
// issued before anything is parked.  Column sums: fixed-order shuffles
// inside the wave, the waves' rows through LDS, one fp32 row per row tile
// into part[M / TILE, N]; reduce_splitk sums the slab.  No atomics; the
// order of a column's sum depends on M alone.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include "mfma_tile.h"

torch::Tensor reduce_splitk(torch::Tensor part, bool out_bf16);

namespace {

#define DD_BK 64
// The output tile edge.  128 (4 waves, 2 blocks per CU) measured 4-5 us
// faster than 256 (8 waves, 1 block per CU) at 65536 x 256 -> 512 and level
// with it at 512 -> 1024 (docs/Kernels.md), so only 128 is instantiated; the
// kernel stays written over TILE as wgrad_kernel is.
#define DD_TILE 128

union DdU16x4 {
  unsigned short u[4];
  unsigned long long ll;
};

// byte offset of bf16 [row][col] in the parked half tile of PW columns:
// 16 B chunk index XOR the row (row pair when two rows share 256 B)
template <int PW>
__device__ __forceinline__ int park_off(int row, int col) {
  constexpr int CPR = PW / 8;         // 16 B chunks per row
  constexpr int RP = 256 / (PW * 2);  // rows per 256 B bank sweep
  const int chunk = (col >> 3) ^ ((row / RP) & (CPR - 1));
  return row * (PW * 2) + (chunk << 4) + (col & 7) * 2;
}

template <int TILE>
__global__ __launch_bounds__(2 * TILE, 2)
void dgrad_drelu_kernel(const unsigned short* __restrict__ A,  // dz_next
                        const unsigned short* __restrict__ W,
                        const unsigned short* __restrict__ Y,
                        unsigned short* __restrict__ DZ,
                        float* __restrict__ part,  // [M / TILE][N]
                        int64_t M, int N, int K) {
  constexpr int FI = 4;            // fragments per wave along M
  constexpr int FJ = TILE / 32;    // ... along N
  constexpr int SC = TILE / 8;     // w staging threads per k-row
  constexpr int NW = TILE / 32;    // waves
  constexpr int PW = TILE / 2;     // columns per epilogue half
  constexpr int OPR = PW / 8;      // octs per parked row
  constexpr int RPS = 2 * TILE / OPR;  // rows per walk sweep
  constexpr int SW = TILE / RPS;       // sweeps per half

  const int tiles_n = (N + TILE - 1) / TILE;
  const int tiles_m = static_cast<int>(M / TILE);
  int tile_m, tile_n;
  if ((tiles_m & 7) == 0) {
    // gemm_bt's XCD-grouped map: the column tiles of one row block land
    // on one XCD and share their rows of dz_next through its L2
    const int c = blockIdx.x & 7;
    const int q = blockIdx.x >> 3;
    tile_n = q % tiles_n;
    tile_m = c + 8 * (q / tiles_n);
  } else {
    tile_m = blockIdx.x / tiles_n;
    tile_n = blockIdx.x - tile_m * tiles_n;
  }
  const int64_t m0 = (int64_t)tile_m * TILE;
  const int n0 = tile_n * TILE;

  __shared__ __attribute__((aligned(16))) unsigned char
      lds_raw[2 * TILE * 128];
  unsigned char* aT = lds_raw;              // [TILE m][64 k] linear swizzle
  unsigned char* wT = lds_raw + TILE * 128;  // [TILE n][64 k] transposed

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = (wave >> 1) * 64;         // M-quadrants of 64
  const int wn = (wave & 1) * (TILE / 2);  // 2 N-halves

  // dz_next staging: row = t >> 1, k seg = (t & 1) * 32
  const int st_r = tid >> 1;
  const int st_k = (tid & 1) * 32;
  // w staging: thread = 4 k-rows x 8 cols
  const int st_kg = (tid / SC) * 4;
  const int st_c = (tid % SC) * 8;
  const bool w_col_ok = (n0 + st_c) < N;  // N % 16 == 0: whole octs

  mfma_f32x4 acc[FI][FJ];
#pragma unroll
  for (int i = 0; i < FI; ++i)
#pragma unroll
    for (int j = 0; j < FJ; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  const int a_row = lane & 15;
  const int a_k = (lane >> 4) * 8;

  bf16x8 ra[4], rw[4];

  auto load_step = [&](int k0) {
    const unsigned short* pa = A + (m0 + st_r) * (int64_t)K + k0 + st_k;
    // K % 16 == 0: whole 8-element vectors are either in or out
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      ra[c] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (k0 + st_k + c * 8 + 8 <= K)
        ra[c] = *reinterpret_cast<const bf16x8*>(pa + c * 8);
    }
    // real branches: a masked lane must not issue the load at all.  The
    // thread's four k-rows start at a multiple of 4, so they are all in
    // or all out.
    const bool w_ok = w_col_ok && (k0 + st_kg) < K;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      rw[rr] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (w_ok)
        rw[rr] = *reinterpret_cast<const bf16x8*>(
            W + (int64_t)(k0 + st_kg + rr) * N + n0 + st_c);
    }
  };

  auto write_step = [&] {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      *reinterpret_cast<bf16x8*>(aT + lds_off_linear(st_r, st_k + c * 8)) =
          ra[c];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      DdU16x4 p{{rw[0][j], rw[1][j], rw[2][j], rw[3][j]}};
      *reinterpret_cast<unsigned long long*>(
          wT + lds_off(st_c + j, st_kg)) = p.ll;
    }
  };

  // fragment (i, j): row wm + i*16 + (lane & 15), columns
  // wn + j*16 + (lane >> 4)*4 + 0..3
  const int e_m = lane & 15;
  const int e_n = (lane >> 4) * 4;
  // walk: one oct of columns, rows w_row + s * RPS
  const int w_row = tid / OPR;
  const int w_oct = tid - w_row * OPR;

  bf16x8 yv[2][SW];
  auto load_y = [&] {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int col = n0 + p * PW + w_oct * 8;
#pragma unroll
      for (int s = 0; s < SW; ++s) {
        yv[p][s] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if (col < N)
          yv[p][s] = *reinterpret_cast<const bf16x8*>(
              Y + (m0 + s * RPS + w_row) * (int64_t)N + col);
      }
    }
  };

  load_step(0);
  for (int k0 = 0; k0 < K; k0 += DD_BK) {
    write_step();
    __syncthreads();
    if (k0 + DD_BK < K) load_step(k0 + DD_BK);  // in flight under MFMA
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
      mfma_bf16x8 a[FI], b[FJ];
#pragma unroll
      for (int i = 0; i < FI; ++i)
        a[i] = *reinterpret_cast<const mfma_bf16x8*>(
            aT + lds_off_linear(wm + i * 16 + a_row, kh * 32 + a_k));
#pragma unroll
      for (int j = 0; j < FJ; ++j)
        b[j] = *reinterpret_cast<const mfma_bf16x8*>(
            wT + lds_off(wn + j * 16 + a_row, kh * 32 + a_k));
#pragma unroll
      for (int i = 0; i < FI; ++i)
#pragma unroll
        for (int j = 0; j < FJ; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              b[j], a[i], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }

  // ---- epilogue ---------------------------------------------------------
  load_y();  // in flight while the accumulators are parked

  float cs[2][8];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int j = 0; j < 8; ++j) cs[p][j] = 0.f;

#pragma unroll
  for (int p = 0; p < 2; ++p) {
    if ((wave & 1) == p) {
#pragma unroll
      for (int i = 0; i < FI; ++i)
#pragma unroll
        for (int j = 0; j < FJ; ++j) {
          DdU16x4 v{{f32_to_bf16(acc[i][j][0]), f32_to_bf16(acc[i][j][1]),
                     f32_to_bf16(acc[i][j][2]), f32_to_bf16(acc[i][j][3])}};
          *reinterpret_cast<unsigned long long*>(
              lds_raw + park_off<PW>(wm + i * 16 + e_m, j * 16 + e_n)) =
              v.ll;
        }
    }
    __syncthreads();
    const int col = n0 + p * PW + w_oct * 8;
#pragma unroll
    for (int s = 0; s < SW; ++s) {
      const int row = s * RPS + w_row;
      const bf16x8 cv = *reinterpret_cast<const bf16x8*>(
          lds_raw + park_off<PW>(row, w_oct * 8));
      bf16x8 out;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool keep = bf16_to_f32(yv[p][s][j]) > 0.f;
        out[j] = keep ? cv[j] : (unsigned short)0;
        if (keep) cs[p][j] += bf16_to_f32(cv[j]);
      }
      if (col < N)
        *reinterpret_cast<bf16x8*>(DZ + (m0 + row) * (int64_t)N + col) = out;
    }
    __syncthreads();
  }

  // column sums: the wave's 64 / OPR rows by shuffles, the waves through
  // LDS in wave order
  float* fsum = reinterpret_cast<float*>(lds_raw);  // [NW][TILE]
#pragma unroll
  for (int p = 0; p < 2; ++p) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = cs[p][j];
#pragma unroll
      for (int off = OPR; off < 64; off <<= 1) v += __shfl_xor(v, off);
      cs[p][j] = v;
    }
    if (lane < OPR) {
      float* dst = fsum + wave * TILE + p * PW + lane * 8;
      reinterpret_cast<f32x4*>(dst)[0] =
          f32x4{cs[p][0], cs[p][1], cs[p][2], cs[p][3]};
      reinterpret_cast<f32x4*>(dst)[1] =
          f32x4{cs[p][4], cs[p][5], cs[p][6], cs[p][7]};
    }
  }
  __syncthreads();
  if (tid < TILE && n0 + tid < N) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) s += fsum[w * TILE + tid];
    part[(int64_t)tile_m * N + n0 + tid] = s;
  }
}

template <int TILE>
std::vector<torch::Tensor> dgrad_drelu_launch(const torch::Tensor& dz_next,
                                              const torch::Tensor& w,
                                              const torch::Tensor& y,
                                              bool dbias_bf16) {
  const int64_t M = dz_next.size(0);
  const int K = static_cast<int>(dz_next.size(1));
  const int N = static_cast<int>(w.size(1));
  auto dz = torch::empty({M, (int64_t)N}, y.options());
  auto part = torch::empty({M / TILE, (int64_t)N},
                           y.options().dtype(torch::kFloat32));
  auto stream = c10::hip::getCurrentHIPStream().stream();
  dim3 grid((M / TILE) * ((N + TILE - 1) / TILE));
  hipLaunchKernelGGL(
      dgrad_drelu_kernel<TILE>, grid, dim3(2 * TILE), 0, stream,
      reinterpret_cast<const unsigned short*>(dz_next.data_ptr()),
      reinterpret_cast<const unsigned short*>(w.data_ptr()),
      reinterpret_cast<const unsigned short*>(y.data_ptr()),
      reinterpret_cast<unsigned short*>(dz.data_ptr()),
      part.data_ptr<float>(), M, N, K);
  return {dz, reduce_splitk(part, dbias_bf16)};
}

}  // namespace

std::vector<torch::Tensor> dgrad_drelu(torch::Tensor dz_next, torch::Tensor w,
                                       torch::Tensor y, bool dbias_bf16) {
  TORCH_CHECK(dz_next.is_cuda() && dz_next.is_contiguous() &&
              dz_next.dim() == 2 &&
              dz_next.scalar_type() == torch::kBFloat16,
              "dz_next must be [M, K] bf16 contiguous");
  TORCH_CHECK(w.is_cuda() && w.is_contiguous() && w.dim() == 2 &&
              w.scalar_type() == torch::kBFloat16,
              "w must be [K, N] bf16 contiguous");
  TORCH_CHECK(y.is_cuda() && y.is_contiguous() && y.dim() == 2 &&
              y.scalar_type() == torch::kBFloat16,
              "y must be [M, N] bf16 contiguous");
  const int64_t M = dz_next.size(0);
  const int64_t K = dz_next.size(1);
  const int64_t N = w.size(1);
  TORCH_CHECK(w.size(0) == K, "K mismatch");
  TORCH_CHECK(y.size(0) == M && y.size(1) == N, "y must be [M, N]");
  TORCH_CHECK(dz_next.device() == w.device() && w.device() == y.device(),
              "operands on different devices");
  TORCH_CHECK(M > 0 && M % 256 == 0 && N > 0 && N % 16 == 0 && K > 0 &&
              K % 16 == 0,
              "dgrad_drelu needs M % 256 == 0, N % 16 == 0, K % 16 == 0");
  TORCH_CHECK(N < (1 << 30) && K < (1 << 30) &&
              (M / 128) * ((N + 127) / 128) < (1LL << 31),
              "dgrad_drelu: shape too large");
  return dgrad_drelu_launch<DD_TILE>(dz_next, w, y, dbias_bf16);
}
