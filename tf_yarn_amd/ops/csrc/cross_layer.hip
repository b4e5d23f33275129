// The DCN-v2 cross layer  y = x0 * (x @ W^T + b) + x  (docs/Kernels.md,
// "Cross layer", has the definition both kernels and the tests share).
//
// cross_fwd_kernel: one MFMA GEMM whose epilogue carries the two [B, D]
// operands the library cannot fuse.
//
//   v32[b, n] = sum_k x[b, k] * W[n, k] + float(bias[n])     fp32
//   y[b, n]   = bf16_rne(float(x0[b, n]) * v32[b, n] + float(x[b, n]))
//   v[b, n]   = bf16_rne(v32[b, n])                          SAVE_V only
//
// Operands.  x [M, K] and W [N, K] (N = K = D) are both K-major, gemm_bt's
// shape, so both take mfma_tile.h's K-major staging, x rows masked at the
// ragged row tile and W rows at the ragged column tile.  128 x 128 tile,
// four waves as 2 x 2 quadrants of 64 x 64, mfma_tile.h's tile map and
// k-step.  The W fragment goes FIRST (dgrad_drelu's order): D's row index
// (four consecutive per lane) is n and its column (lane & 15) is m, so a
// lane holds four adjacent columns of one output row.
//
// Epilogue.  y needs the fp32 v32, so the accumulators are parked as fp32:
// a half tile of 128 rows x 64 columns is 32 KB, exactly the two operand
// images, which are free after the k-loop's last barrier.  Per column half
// the two waves that own it park one f32x4 per fragment (16 B chunks
// XOR-swizzled by row), then ALL threads walk the half in
// bias_relu_bwd_dbpart8_body's row/oct map: a thread owns one oct of
// columns, takes x0 and x as bf16x8 from memory (issued before the park,
// in flight under it) and its two f32x4 from LDS, and stores y (and v) as
// bf16x8.  No 2-byte scatter.
//
// cross_bwd_pre_kernel: the elementwise front of the backward in one
// streaming pass, three reads and two writes per element:
//
//   dz  = bf16_rne(float(g) * float(x0))
//   dx0 = bf16_rne(float(g) * float(v))
//   part[block][n] = sum over the block's rows of float(dz[., n])
//
// in the same row/oct map; the block's row slots are summed through LDS in
// slot order into ONE fp32 row per block and reduce_splitk finishes the
// column sums.  No atomics; the grid, and so a column's summation order,
// depends on B and D alone.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <tuple>
#include "mfma_tile.h"

torch::Tensor reduce_splitk(torch::Tensor part, bool out_bf16);

namespace {

// the fp32 epilogue arithmetic stays scalar instructions
#define CL_KERNEL __attribute__((target("no-packed-fp32-ops")))

#define CL_BK 64
#define CL_TILE 128
#define CL_PW 64     // columns per parked half
#define CL_MIN_D 16
#define CL_MAX_D 1024
// rows a bwd_pre thread has in flight: three operands per row, so 2 keeps
// it at 85 VGPRs (5 waves per SIMD); 4 took 129 (3 waves)
#define CL_ROWS 2

// __syncthreads(), spelled out: under CL_KERNEL's target attribute only
// forced-inline helpers are inlined, and the barrier should not be a call
__device__ __forceinline__ void block_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// byte offset of fp32 [row][col] in the parked half tile: 256 B rows, the
// 16 B chunk index XOR the row
__device__ __forceinline__ int park_off32(int row, int col) {
  return row * 256 + ((((col >> 2) ^ row) & 15) << 4) + (col & 3) * 4;
}

template <bool SAVE_V>
__global__ CL_KERNEL __launch_bounds__(2 * CL_TILE, 3)
void cross_fwd_kernel(const unsigned short* __restrict__ X0,
                      const unsigned short* __restrict__ X,
                      const unsigned short* __restrict__ W,
                      const unsigned short* __restrict__ bias,
                      unsigned short* __restrict__ Y,
                      unsigned short* __restrict__ V,
                      int64_t M, int D, int64_t ld0, int64_t ldx) {
  constexpr int TILE = CL_TILE;
  constexpr int FI = 4, FJ = 4;        // 64 x 64 per wave
  constexpr int OPR = CL_PW / 8;       // octs per parked row
  constexpr int RPS = 2 * TILE / OPR;  // rows per walk sweep
  constexpr int SW = TILE / RPS;       // sweeps per half

  const int tiles_n = (D + TILE - 1) / TILE;
  const int tiles_m = static_cast<int>((M + TILE - 1) / TILE);
  int tile_m, tile_n;
  xcd_tile_map(tiles_m, tiles_n, tile_m, tile_n);  // shares x's rows
  const int64_t m0 = (int64_t)tile_m * TILE;
  const int n0 = tile_n * TILE;

  __shared__ __attribute__((aligned(16))) unsigned char
      lds_raw[2 * TILE * 128];
  unsigned char* xT = lds_raw;               // [TILE m][64 k]
  unsigned char* wT = lds_raw + TILE * 128;  // [TILE n][64 k]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = (wave >> 1) * 64;
  const int wn = (wave & 1) * 64;

  const int st_r = tid >> 1;
  const int st_k = (tid & 1) * 32;
  const bool x_row_ok = (m0 + st_r) < M;  // ragged M
  const bool w_row_ok = (n0 + st_r) < D;  // ragged N

  mfma_f32x4 acc[FI][FJ];
  zero_acc(acc);

  bf16x8 rx[4], rw[4];
  // the lambda carries the kernel's target attribute, or it is not inlined
  auto load_step = [&](int k0) CL_KERNEL {
    stage_kmajor_load(rx, X + (m0 + st_r) * ldx + k0 + st_k, x_row_ok,
                      k0 + st_k, D);
    stage_kmajor_load(rw, W + (int64_t)(n0 + st_r) * D + k0 + st_k, w_row_ok,
                      k0 + st_k, D);
  };

  load_step(0);
  for (int k0 = 0; k0 < D; k0 += CL_BK) {
    stage_kmajor_write(xT, rx, st_r, st_k);
    stage_kmajor_write(wT, rw, st_r, st_k);
    block_sync();
    if (k0 + CL_BK < D) load_step(k0 + CL_BK);  // in flight under MFMA
    // the W fragment goes first (header comment)
    mfma_kstep<FI, FJ, lds_off_linear, lds_off_linear, true>(acc, xT, wT, wm,
                                                             wn, lane);
    block_sync();
  }

  // ---- epilogue ---------------------------------------------------------
  // fragment (i, j): row wm + i*16 + f_col, columns wn + j*16 + f_row4 + 0..3
  int f_col, f_row4;
  frag_pos(lane, f_col, f_row4);
  const int w_row = tid / OPR;
  const int w_oct = tid - w_row * OPR;

#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int col = n0 + p * CL_PW + w_oct * 8;
    const bool col_ok = col < D;  // D % 16 == 0: whole octs
    bf16x8 x0v[SW], xv[SW];
    bf16x8 bv = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    if (col_ok) bv = *reinterpret_cast<const bf16x8*>(bias + col);
#pragma unroll
    for (int s = 0; s < SW; ++s) {
      const int64_t row = m0 + s * RPS + w_row;
      x0v[s] = xv[s] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (col_ok && row < M) {
        x0v[s] = *reinterpret_cast<const bf16x8*>(X0 + row * ld0 + col);
        xv[s] = *reinterpret_cast<const bf16x8*>(X + row * ldx + col);
      }
    }
    if ((wave & 1) == p) {
#pragma unroll
      for (int i = 0; i < FI; ++i)
#pragma unroll
        for (int j = 0; j < FJ; ++j)
          *reinterpret_cast<f32x4*>(
              lds_raw + park_off32(wm + i * 16 + f_col, j * 16 + f_row4)) =
              f32x4{acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
    }
    block_sync();
#pragma unroll
    for (int s = 0; s < SW; ++s) {
      const int lrow = s * RPS + w_row;
      const int64_t row = m0 + lrow;
      const f32x4 lo = *reinterpret_cast<const f32x4*>(
          lds_raw + park_off32(lrow, w_oct * 8));
      const f32x4 hi = *reinterpret_cast<const f32x4*>(
          lds_raw + park_off32(lrow, w_oct * 8 + 4));
      bf16x8 yo, vo;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float v32 = (j < 4 ? lo[j & 3] : hi[j & 3]) +
                          bf16_to_f32(bv[j]);
        yo[j] = f32_to_bf16(bf16_to_f32(x0v[s][j]) * v32 +
                            bf16_to_f32(xv[s][j]));
        if (SAVE_V) vo[j] = f32_to_bf16(v32);
      }
      if (col_ok && row < M) {
        *reinterpret_cast<bf16x8*>(Y + row * D + col) = yo;
        if (SAVE_V) *reinterpret_cast<bf16x8*>(V + row * D + col) = vo;
      }
    }
    block_sync();
  }
}

__global__ CL_KERNEL __launch_bounds__(MIYARN_BLOCK, 4)
void cross_bwd_pre_kernel(const unsigned short* __restrict__ G,
                          const unsigned short* __restrict__ X0,
                          const unsigned short* __restrict__ V,
                          unsigned short* __restrict__ DZ,
                          unsigned short* __restrict__ DX0,
                          float* __restrict__ part,  // [gridDim.x][cols]
                          int64_t rows, int cols, int64_t ldg, int64_t ld0,
                          int64_t ldv) {
  // blockDim.x == rpb * octs: every thread has a slot and an oct
  const int octs = cols >> 3;
  const int rpb = blockDim.x / octs;
  const int rid = threadIdx.x / octs;
  const int q = threadIdx.x - rid * octs;
  const int c = q * 8;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;

  const int64_t slot = (int64_t)blockIdx.x * rpb + rid;
  const int64_t row_stride = (int64_t)gridDim.x * rpb * CL_ROWS;
  for (int64_t r0 = slot * CL_ROWS; r0 < rows; r0 += row_stride) {
    const int nr = rows - r0 < CL_ROWS ? (int)(rows - r0) : CL_ROWS;
    bf16x8 gv[CL_ROWS], av[CL_ROWS], vv[CL_ROWS];
#pragma unroll
    for (int rr = 0; rr < CL_ROWS; ++rr)
      if (rr < nr) {
        gv[rr] = *reinterpret_cast<const bf16x8*>(G + (r0 + rr) * ldg + c);
        av[rr] = *reinterpret_cast<const bf16x8*>(X0 + (r0 + rr) * ld0 + c);
        vv[rr] = *reinterpret_cast<const bf16x8*>(V + (r0 + rr) * ldv + c);
      }
#pragma unroll
    for (int rr = 0; rr < CL_ROWS; ++rr)
      if (rr < nr) {
        bf16x8 dz, dx0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float g = bf16_to_f32(gv[rr][j]);
          dz[j] = f32_to_bf16(g * bf16_to_f32(av[rr][j]));
          dx0[j] = f32_to_bf16(g * bf16_to_f32(vv[rr][j]));
          acc[j] += bf16_to_f32(dz[j]);  // of the ROUNDED dz
        }
        *reinterpret_cast<bf16x8*>(DZ + (r0 + rr) * cols + c) = dz;
        *reinterpret_cast<bf16x8*>(DX0 + (r0 + rr) * cols + c) = dx0;
      }
  }

  // the block's slots, in slot order, into one row
  __shared__ __attribute__((aligned(16))) float fsum[MIYARN_BLOCK * 8];
  float* mine = fsum + (rid * octs + q) * 8;
  reinterpret_cast<f32x4*>(mine)[0] = f32x4{acc[0], acc[1], acc[2], acc[3]};
  reinterpret_cast<f32x4*>(mine)[1] = f32x4{acc[4], acc[5], acc[6], acc[7]};
  block_sync();
  if (rid == 0) {
    f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < rpb; ++s) {
      const float* src = fsum + (s * octs + q) * 8;
      lo += reinterpret_cast<const f32x4*>(src)[0];
      hi += reinterpret_cast<const f32x4*>(src)[1];
    }
    float* dst = part + (int64_t)blockIdx.x * cols + c;
    reinterpret_cast<f32x4*>(dst)[0] = lo;
    reinterpret_cast<f32x4*>(dst)[1] = hi;
  }
}

// [B, D] bf16 with unit column stride, rows a multiple of 8 elements and at
// least their own width apart and a 16 B aligned base: what the 16 B loads
// need
bool rows_ok(const torch::Tensor& t) {
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

bool dim_ok(int64_t d) {
  return d % 16 == 0 && d >= CL_MIN_D && d <= CL_MAX_D;
}

const unsigned short* cptr(const torch::Tensor& t) {
  return reinterpret_cast<const unsigned short*>(t.data_ptr());
}
unsigned short* mptr(torch::Tensor& t) {
  return reinterpret_cast<unsigned short*>(t.data_ptr());
}

}  // namespace

// True when cross_bwd_pre (and cross_fwd, for x0 and x) reads these rows in
// place: the layout test of their TORCH_CHECK, for the caller that would
// rather copy than raise.
bool cross_rows_ok(torch::Tensor t) { return rows_ok(t); }

bool cross_layer_ok(torch::Tensor x0, torch::Tensor x, torch::Tensor weight,
                    torch::Tensor bias) {
  if (!(rows_ok(x0) && rows_ok(x) && x0.sizes() == x.sizes())) return false;
  const int64_t D = x.size(1);
  return dim_ok(D) && weight.is_cuda() && bias.is_cuda() &&
         weight.scalar_type() == torch::kBFloat16 &&
         bias.scalar_type() == torch::kBFloat16 && weight.dim() == 2 &&
         weight.size(0) == D && weight.size(1) == D &&
         weight.is_contiguous() && bias.dim() == 1 && bias.size(0) == D &&
         bias.is_contiguous() && miyarn_aligned(weight.data_ptr(), 16) &&
         miyarn_aligned(bias.data_ptr(), 16) && x0.device() == x.device() &&
         x.device() == weight.device() && weight.device() == bias.device() &&
         (x.size(0) + CL_TILE - 1) / CL_TILE * ((D + CL_TILE - 1) / CL_TILE) <
             (1LL << 31);
}

std::tuple<torch::Tensor, c10::optional<torch::Tensor>> cross_fwd(
    torch::Tensor x0, torch::Tensor x, torch::Tensor weight,
    torch::Tensor bias, bool save_v) {
  TORCH_CHECK(cross_layer_ok(x0, x, weight, bias),
              "cross_fwd needs bf16 x0, x [B, D] (unit column stride, row "
              "stride % 8 == 0, 16 B aligned), weight [D, D] and bias [D] "
              "contiguous on one GPU, D % 16 == 0, 16 <= D <= 1024");
  const int64_t M = x.size(0);
  const int D = static_cast<int>(x.size(1));
  auto y = torch::empty({M, (int64_t)D}, x.options());
  c10::optional<torch::Tensor> v;
  if (save_v) v = torch::empty({M, (int64_t)D}, x.options());
  if (M == 0) return {y, v};
  auto stream = c10::hip::getCurrentHIPStream().stream();
  dim3 grid(((M + CL_TILE - 1) / CL_TILE) * ((D + CL_TILE - 1) / CL_TILE));
  auto* kern = save_v ? cross_fwd_kernel<true> : cross_fwd_kernel<false>;
  hipLaunchKernelGGL(kern, grid, dim3(2 * CL_TILE), 0, stream, cptr(x0),
                     cptr(x), cptr(weight), cptr(bias), mptr(y),
                     save_v ? mptr(*v) : nullptr, M, D, row_ld(x0),
                     row_ld(x));
  return {y, v};
}

std::vector<torch::Tensor> cross_bwd_pre(torch::Tensor g, torch::Tensor x0,
                                         torch::Tensor v) {
  TORCH_CHECK(rows_ok(g) && rows_ok(x0) && rows_ok(v) &&
              g.sizes() == x0.sizes() && g.sizes() == v.sizes() &&
              g.device() == x0.device() && g.device() == v.device() &&
              dim_ok(g.size(1)),
              "cross_bwd_pre needs bf16 g, x0, v [B, D] on one GPU (unit "
              "column stride, row stride % 8 == 0, 16 B aligned), "
              "D % 16 == 0, 16 <= D <= 1024");
  const int64_t B = g.size(0);
  const int D = static_cast<int>(g.size(1));
  auto dz = torch::empty({B, (int64_t)D}, g.options());
  auto dx0 = torch::empty({B, (int64_t)D}, g.options());
  if (B == 0)
    return {dz, dx0, torch::zeros({(int64_t)D}, g.options())};
  const int octs = D / 8;                             // 2 .. 128
  const int rpb = std::max(1, MIYARN_BLOCK / octs);   // row slots per block
  const int64_t rows_per_block = (int64_t)rpb * CL_ROWS;
  const int grid = static_cast<int>(std::min<int64_t>(
      (B + rows_per_block - 1) / rows_per_block, MIYARN_MAX_BLOCKS));
  auto part = torch::empty({(int64_t)grid, (int64_t)D},
                           g.options().dtype(torch::kFloat32));
  auto stream = c10::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(cross_bwd_pre_kernel, dim3(grid), dim3(rpb * octs), 0,
                     stream, cptr(g), cptr(x0), cptr(v), mptr(dz), mptr(dx0),
                     part.data_ptr<float>(), B, D, row_ld(g), row_ld(x0),
                     row_ld(v));
  return {dz, dx0, reduce_splitk(part, true)};
}
