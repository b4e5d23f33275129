// Split-K MFMA weight-gradient kernel for tall, narrow outputs on MI355X
// (gfx950).
//
// dW[N, M] = sum_b dy[b, n] * x[b, m]  with dy [B, N], x [B, M] bf16
// row-major, where one side r = min(N, M) is narrow (8..128) and the other
// Wd = max(N, M) is at most 1024: the low-rank cross layer's dU [D, r] and
// dV [r, D], the last layer of a bottom MLP, any projection to a small
// width, at ANY batch size.  wgrad.hip needs N % 128 == 0 and B % 64 == 0
// and its 128^2 / 256^2 tiles would spend most of their MFMAs on padding.
//
// Work split.  A block of 256 threads owns 128 wide-side columns and ALL
// RP narrow columns (RP = r padded to 32, 64 or 128).  Wave w owns wide
// columns 32w .. 32w+31: 2 x RP/16 accumulator fragments, 64 fp32
// registers at RP = 128.  The narrow operand is staged once per block and
// read by all four waves; the wide operand is read from memory once
// overall.  Grid (splitk, ceil(Wd / 128)), slab-major as in wgrad.hip: the
// tiles of one k-slab share an XCD's L2 for the narrow rows they all read.
// Each block reduces a contiguous chunk of 64-row k-steps into
// part[slab][N][M] in fp32 (no atomics); reduce_splitk sums the slabs.
//
// k-loop.  Both operands are k-strided, so both take mfma_tile.h's strided
// register staging (four k-rows x one oct of columns per thread, packed
// b64 transposed writes into a [col][64 k] image under lds_off) and the
// shared mfma_kstep; the next step's global loads are issued before the
// MFMA phase.  Register staging rather than LDS-DMA because of the k
// tail: a row >= B, or past the slab's end, must contribute real zeros to
// EVERY column, and a masked register load is a zero where a masked DMA
// lane leaves whatever the buffer held.  Column tails are zeroed the same
// way (whole octs: r % 8 == 0, Wd % 8 == 0).  One 16 KB wide image plus
// one RP * 128 B narrow image: at most 32 KB.
//
// Orientation.  The MFMA's first operand indexes D's rows, and a lane
// holds four consecutive rows of one column.  x always goes first: the
// four registers are then four consecutive m of one n, one 16 B store
// into the slab in dW's own [N][M] layout, in both orientations.
// NARROW_IS_N says which operand is the narrow one (dy for dV-like
// shapes, x for dU-like ones) and which way the epilogue indexes.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include "mfma_tile.h"

torch::Tensor reduce_splitk(torch::Tensor part, bool out_bf16);

namespace {

// no fp32 arithmetic outside the MFMAs; kept with the neighbours' attribute
#define WN_KERNEL __attribute__((target("no-packed-fp32-ops")))

#define WN_BK 64
#define WN_TILE 128      // wide columns per block
#define WN_MIN_R 8
#define WN_MAX_R 128
#define WN_MAX_WIDE 1024
// blocks of one launch: two resident per CU
#define WN_BLOCK_BUDGET 512
// most slabs, of the auto plan and of an explicit splitk
#define WN_MAX_SPLITK 256

// __syncthreads(), spelled out (cross_layer.hip has the reason)
__device__ __forceinline__ void block_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// stage_strided_load with a per-row k mask: the thread's four k-rows are
// in range while rr < rows_left (B is arbitrary here, so they are not all
// in or all out).  Real branches: a masked lane issues no load.
__device__ __forceinline__ void stage_tail_load(bf16x8 (&r)[4],
                                                const unsigned short* p,
                                                int64_t ld, bool col_ok,
                                                int64_t rows_left) {
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    r[rr] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    if (col_ok && rr < rows_left)
      r[rr] = *reinterpret_cast<const bf16x8*>(p + rr * ld);
  }
}

template <int RP, bool NARROW_IS_N>
__global__ __launch_bounds__(256) WN_KERNEL
void wgrad_narrow_kernel(const unsigned short* __restrict__ dy,
                         const unsigned short* __restrict__ x,
                         float* __restrict__ part,
                         int64_t B, int N, int M, int64_t chunk) {
  constexpr int FW = 2;         // fragments per wave along the wide side
  constexpr int FR = RP / 16;   // ... along the narrow side
  constexpr int SCN = RP / 8;   // staging threads per narrow k-row

  const unsigned short* wide = NARROW_IS_N ? x : dy;
  const unsigned short* nar = NARROW_IS_N ? dy : x;
  const int Wd = NARROW_IS_N ? M : N;
  const int r = NARROW_IS_N ? N : M;
  const int w0 = blockIdx.y * WN_TILE;
  const int64_t k_begin = (int64_t)blockIdx.x * chunk;
  const int64_t k_end = min(B, k_begin + chunk);

  __shared__ __attribute__((aligned(16))) unsigned char
      lds_raw[(WN_TILE + RP) * 128];
  unsigned char* wideT = lds_raw;                  // [128 col][64 k]
  unsigned char* narT = lds_raw + WN_TILE * 128;   // [RP col][64 k]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wm = (tid >> 6) * 32;

  // staging maps: 16 k-groups of 4 rows x (16 | SCN) octs; the first
  // 2 * RP threads (whole waves) also stage the narrow operand
  const int sw_kg = (tid >> 4) * 4;
  const int sw_c = (tid & 15) * 8;
  const bool w_col_ok = (w0 + sw_c) < Wd;
  const bool n_stager = tid < 16 * SCN;
  const int sn_kg = (tid / SCN) * 4;
  const int sn_c = (tid % SCN) * 8;
  const bool n_col_ok = n_stager && sn_c < r;

  mfma_f32x4 acc[FW][FR];
  zero_acc<FW, FR>(acc);

  bf16x8 rw[4], rn[4];
  {
    const int64_t kw = k_begin + sw_kg, kn = k_begin + sn_kg;
    stage_tail_load(rw, wide + kw * Wd + w0 + sw_c, Wd, w_col_ok,
                    k_end - kw);
    stage_tail_load(rn, nar + kn * r + sn_c, r, n_col_ok, k_end - kn);
  }
  for (int64_t k0 = k_begin; k0 < k_end; k0 += WN_BK) {
    stage_strided_write(wideT, rw, sw_c, sw_kg);
    if (n_stager) stage_strided_write(narT, rn, sn_c, sn_kg);
    block_sync();
    if (k0 + WN_BK < k_end) {  // in flight under the MFMA phase
      const int64_t kw = k0 + WN_BK + sw_kg, kn = k0 + WN_BK + sn_kg;
      stage_tail_load(rw, wide + kw * Wd + w0 + sw_c, Wd, w_col_ok,
                      k_end - kw);
      stage_tail_load(rn, nar + kn * r + sn_c, r, n_col_ok, k_end - kn);
    }
    // acc[i][j]: wide fragment i, narrow fragment j; x first (see above)
    mfma_kstep<FW, FR, lds_off, lds_off, !NARROW_IS_N>(acc, wideT, narT, wm,
                                                       0, lane);
    block_sync();
  }

  // ---- epilogue: one 16 B store per fragment into dW's own layout -------
  float* out = part + (int64_t)blockIdx.x * N * M;
  int f_col, f_row4;
  frag_pos(lane, f_col, f_row4);
#pragma unroll
  for (int i = 0; i < FW; ++i)
#pragma unroll
    for (int j = 0; j < FR; ++j) {
      // D rows (f_row4 + reg) index x's columns, D's column indexes dy's
      const int wc = w0 + wm + i * 16;
      const int n = NARROW_IS_N ? j * 16 + f_col : wc + f_col;
      const int m = NARROW_IS_N ? wc + f_row4 : j * 16 + f_row4;
      // m % 4 == 0 and M % 4 == 0: the four are in or out together
      if (n < N && m < M)
        *reinterpret_cast<mfma_f32x4*>(out + (int64_t)n * M + m) = acc[i][j];
    }
}

template <int RP, bool NARROW_IS_N>
void wn_launch(const torch::Tensor& dy, const torch::Tensor& x,
               torch::Tensor& part, int64_t chunk, int tiles) {
  auto stream = c10::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL((wgrad_narrow_kernel<RP, NARROW_IS_N>),
                     dim3(part.size(0), tiles), dim3(256), 0, stream,
                     reinterpret_cast<unsigned short*>(dy.data_ptr()),
                     reinterpret_cast<unsigned short*>(x.data_ptr()),
                     part.data_ptr<float>(), dy.size(0),
                     static_cast<int>(dy.size(1)),
                     static_cast<int>(x.size(1)), chunk);
}

template <bool NARROW_IS_N>
void wn_dispatch(int r, const torch::Tensor& dy, const torch::Tensor& x,
                 torch::Tensor& part, int64_t chunk, int tiles) {
  if (r <= 32) wn_launch<32, NARROW_IS_N>(dy, x, part, chunk, tiles);
  else if (r <= 64) wn_launch<64, NARROW_IS_N>(dy, x, part, chunk, tiles);
  else wn_launch<128, NARROW_IS_N>(dy, x, part, chunk, tiles);
}

}  // namespace

torch::Tensor wgrad_narrow(torch::Tensor dy, torch::Tensor x, int64_t splitk,
                           bool out_bf16) {
  TORCH_CHECK(dy.is_cuda() && dy.is_contiguous() && dy.dim() == 2 &&
              dy.scalar_type() == torch::kBFloat16,
              "wgrad_narrow: dy must be [B, N] bf16 contiguous");
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 2 &&
              x.scalar_type() == torch::kBFloat16,
              "wgrad_narrow: x must be [B, M] bf16 contiguous");
  const int64_t B = dy.size(0);
  TORCH_CHECK(x.size(0) == B && B >= 1,
              "wgrad_narrow: dy and x need the same batch >= 1");
  const int64_t N = dy.size(1), M = x.size(1);
  const int64_t r = std::min(N, M), wd = std::max(N, M);
  TORCH_CHECK(r % 8 == 0 && r >= WN_MIN_R && r <= WN_MAX_R && wd % 8 == 0 &&
              wd <= WN_MAX_WIDE,
              "wgrad_narrow needs min(N, M) % 8 == 0 in [", WN_MIN_R, ", ",
              WN_MAX_R, "] and max(N, M) % 8 == 0, <= ", WN_MAX_WIDE,
              "; got N = ", N, ", M = ", M);
  TORCH_CHECK(miyarn_aligned(dy.data_ptr(), 16) &&
              miyarn_aligned(x.data_ptr(), 16),
              "wgrad_narrow needs 16-byte-aligned operands");
  const int tiles = static_cast<int>((wd + WN_TILE - 1) / WN_TILE);
  // Auto plan, from the sweep in docs/Kernels.md: about two resident
  // blocks per CU (128 slabs at four tiles, 256 at two), and at least two
  // k-steps per slab so that a block has a load to keep in flight (one-step
  // slabs measured 23 us where two-step slabs took 16 at B = 4096).  An
  // explicit splitk (tests, sweeps) is only capped.
  if (splitk <= 0)
    splitk = std::max<int64_t>(
        1, std::min<int64_t>(WN_BLOCK_BUDGET / tiles, B / (2 * WN_BK)));
  splitk = std::min<int64_t>(splitk, WN_MAX_SPLITK);
  // whole 64-row k-steps per slab, and no empty slab
  const int64_t chunk =
      ((B + splitk - 1) / splitk + WN_BK - 1) / WN_BK * WN_BK;
  splitk = (B + chunk - 1) / chunk;
  auto part = torch::empty({splitk, N, M},
                           dy.options().dtype(torch::kFloat32));
  if (N <= M)
    wn_dispatch<true>(static_cast<int>(r), dy, x, part, chunk, tiles);
  else
    wn_dispatch<false>(static_cast<int>(r), dy, x, part, chunk, tiles);
  return reduce_splitk(part, out_bf16);
}
