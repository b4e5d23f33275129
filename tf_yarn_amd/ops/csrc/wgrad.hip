// Split-K MFMA weight-gradient kernel for MI355X (gfx950), one template
// over the output tile edge: 128 (v3) and 256 (v4).
//
// dW[N, M] = sum_b dy[b, n] * x[b, m]  with dy [B, N], x [B, M] bf16
// row-major and B ~ 65536: the "reduction GEMM" shape hipBLASLt runs at
// 140-380 TF on this chip (measured, scripts/micro_gemm.py) because its
// split-K solutions are weak.
//
// Ladder (B=65536, 1024x432 / 512x1024):
//  * v2, 64x64 tiles, padded LDS, no prefetch (removed): 118-129 TF —
//    redundant operand traffic (dy re-read tiles_m times, x re-read
//    tiles_n times) plus LDS write conflicts bound it.
//  * v3, TILE=128: halves that traffic (~1 GB for the 1024x432 layer);
//    swizzled LDS, masked column edges (M need not divide the tile, so
//    the model's 432-wide first layer is served directly), next-step
//    global loads issued under the MFMA phase.  Still traffic-bound.
//  * v4, TILE=256: halves it again (~0.5 GB), the regime where the
//    B-sweep says the structure already matches hipBLASLt: 581/655 TF,
//    633/738 TF with the slab-major grid below.
//
// Geometry: 2*TILE threads = TILE/32 waves in (TILE/64)(N) x 2(M)
// quadrants, each wave 64 x TILE/2 = 4 x TILE/32 fragments (TILE=256:
// 128 fp32 acc/lane — ~2 waves/SIMD, 1 block/CU).  Two k-loops share the
// template (see wgrad_kernel): the default fills row-major [64 k][128
// col] LDS images by LDS-DMA into two buffers and reads the fragments
// with the transposing LDS read; the register-staged control holds both
// operands TRANSPOSED as [n][64 k] / [m][64 k] rows of 128 B under
// mfma_tile.h's combined swizzle (packed b64 transposed writes and b128
// fragment reads both conflict-light).  Each split-K block reduces
// its contiguous k-chunk into an fp32 slab part[sk][N][M] (atomic-free,
// deterministic); reduce_splitk sums the slabs.
//
// XCD-aware slab-major mapping: the dispatcher places linear block b on
// XCD b % 8 (MI355X_MICROARCH "Workgroup dispatch").  With grid =
// (splitk, tiles), linear id = slab + splitk*tile, so all tiles of one
// k-slab land on XCD slab%8 and share their dy/x column reads through
// that XCD's 4 MB L2 (the old (tiles, splitk) grid put every tile of a
// slab on a DIFFERENT XCD — zero reuse; operand re-reads made the kernel
// HBM-bound at ~5.6 TB/s).
//
// Double-buffering post-mortem (round 2): two LDS buffer pairs with one
// barrier per k-step were tried twice at TILE=256 — runtime buffer select
// (537 TF) and a 2x-unrolled constant-offset pipeline (544/580 TF) — and
// BOTH lost to this single-buffered loop (581/655 TF measured).  At 2
// waves/SIMD the two-barrier alternation keeps the MFMA and LDS-staging
// phases of the co-resident waves interleaved; the "saved" barrier was
// not the bottleneck.  Both attempts kept the register staging and its
// transposed write pass.  The LDS-DMA loop that replaced it as the default
// drops both (no staging VGPRs, no ds_write, no vmcnt(0)-before-write)
// and does win with two buffers: 83/85 us against 100/99 us at TILE=256
// and 50 against 57 us at TILE=128 (reduce included,
// profiles/r12_wgrad_glds.md).

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include "mfma_tile.h"

torch::Tensor reduce_splitk(torch::Tensor part, bool out_bf16);

namespace {

#define WG_BK 64

union U16x4 {
  unsigned short u[4];
  unsigned long long ll;
};

// LDS-DMA staging (GLDS = true) constants; mirrored by
// tests/wgrad_image.py through wgrad_glds_layout().
constexpr int WG_IMG_COLS = 128;                 // columns of one image
constexpr int WG_IMG_BYTES = WG_BK * 2 * WG_IMG_COLS;  // 16 KB
constexpr int WG_FILL_ROWS = 4;   // image rows per DMA wave-instruction
constexpr int WG_FILLS_PER_WAVE = 8;

typedef __attribute__((ext_vector_type(4))) __bf16 mfma_bf16x4;
#define WG_LDS_AS __attribute__((address_space(3)))

// GLDS = false: the register-staged k-loop (global -> VGPR -> transposed
// ds_write_b64 -> barrier -> ds_read_b128 -> MFMA -> barrier).
// GLDS = true: both operands go global -> LDS by 16 B LDS-DMA into two
// buffers of row-major [64 k][128 col] images (mfma_tile.h, lds_off_tr)
// and the fragments come from transposed LDS reads; one barrier per
// k-step, no staging registers, no LDS write pass.  Same k order, same
// MFMA operand registers, same split plan: bit-identical dW.
template <int TILE, bool GLDS>
__global__ __launch_bounds__(2 * TILE)
void wgrad_kernel(const unsigned short* __restrict__ dy,
                  const unsigned short* __restrict__ x,
                  float* __restrict__ part,
                  int64_t B, int N, int M, int64_t chunk) {
  constexpr int FN = 4;          // fragments per wave along N
  constexpr int FM = TILE / 32;  // ... along M
  constexpr int SC = TILE / 8;   // staging threads per k-row

  const int tiles_m = (M + TILE - 1) / TILE;
  const int tile_n = blockIdx.y / tiles_m;
  const int tile_m = blockIdx.y - tile_n * tiles_m;
  const int n0 = tile_n * TILE;
  const int m0 = tile_m * TILE;
  const int64_t k_begin = (int64_t)blockIdx.x * chunk;
  const int64_t k_end = min(B, k_begin + chunk);

  // one array for everything in LDS (a second __shared__ object beside
  // an LDS-DMA target can make the compiler drain the DMA queue before
  // every fragment read)
  __shared__ __attribute__((aligned(16))) unsigned char
      lds_raw[(GLDS ? 4 : 2) * TILE * 128];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wn = (wave >> 1) * 64;          // N-quadrants of 64
  const int wm = (wave & 1) * (TILE / 2);   // 2 M-halves

  mfma_f32x4 acc[FN][FM];
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FM; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  if constexpr (GLDS) {
    constexpr int NI = TILE / WG_IMG_COLS;     // images per operand
    constexpr int OPB = NI * WG_IMG_BYTES;     // one operand, one k-step
    constexpr int BUFB = 2 * OPB;              // one buffer: dy then x
    constexpr int WPO = TILE / 64;             // filling waves per operand

    // ---- fill map: wave w DMAs 8 consecutive 4-row groups of one
    // operand; lane L lands on physical chunk L%16 of row r0 + L/16 and
    // so fetches logical chunk (L%16) ^ swz(row)
    const int uw = __builtin_amdgcn_readfirstlane(wave);
    const int f_op = uw / WPO;                          // 0: dy, 1: x
    const int f_grp = (uw % WPO) * WG_FILLS_PER_WAVE;   // of NI*16 groups
    const int f_img = f_grp / 16;
    const int f_r0 = (f_grp % 16) * WG_FILL_ROWS;
    const unsigned short* f_ptr = f_op ? x : dy;
    const int f_ld = f_op ? M : N;
    // chunk clamp: a ragged last x tile (M % 8 == 0) re-fetches its last
    // valid chunk; columns >= M only feed accumulator columns the
    // epilogue masks.  dy never clamps (N % TILE == 0).
    const int f_cmax = f_ld / 8 - 1;
    const int f_c0 = (f_op ? m0 : n0) / 8 + f_img * 16;
    const int f_row = f_r0 + (lane >> 4);
    const unsigned short* f_src[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int row = f_row + WG_FILL_ROWS * t;
      const int ch = min(f_c0 + ((lane & 15) ^ lds_swz_tr(row)), f_cmax);
      f_src[t] = f_ptr + (int64_t)row * f_ld + ch * 8;
    }
    const unsigned f_dst =
        (unsigned)(uintptr_t)(WG_LDS_AS unsigned char*)lds_raw +
        f_op * OPB + f_img * WG_IMG_BYTES + f_r0 * 256;

    // The DMA is issued from an asm statement, not through
    // __builtin_amdgcn_global_load_lds: with the builtin the compiler
    // counts the DMA as a pending LDS store and puts s_waitcnt vmcnt(0)
    // ahead of the first fragment read of the OTHER buffer in every
    // k-step (seen in the .s), which serialises fill and compute.  The
    // statement writes M0 (the wave-uniform LDS destination; the hardware
    // adds lane * 16) in the same string that uses it and restores it;
    // publish() below does the waiting.
    auto stage = [&](int64_t k0, int bufoff) {
      const int64_t koff = k0 * f_ld;
#pragma unroll
      for (int t = 0; t < WG_FILLS_PER_WAVE; ++t) {
        // rows 16 apart share their swizzle term
        const unsigned short* src =
            f_src[t & 3] + koff + (int64_t)(t >> 2) * 16 * f_ld;
        const unsigned dst = f_dst + bufoff + t * WG_FILL_ROWS * 256;
        unsigned keep;
        asm volatile(
            "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
            "global_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
            : "=&s"(keep)
            : "v"(src), "s"(dst)
            : "memory");
      }
    };

    // ---- fragment map: lane 4q+p of group g reads k-rows 8g + 4h + q
    // (h = 0, 1), chunk 2c + (p>>1), bytes 8*(p&1); the fragment's column
    // block c enters by XOR on bits 5..7, so one base per h serves all
    const int t_q = (lane >> 2) & 3, t_p = lane & 3, t_g = lane >> 4;
    int a_base[2], b_base[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = 8 * t_g + 4 * h + t_q;
      const int o = lds_off_tr(row, t_p >> 1) + 8 * (t_p & 1);
      a_base[h] = (o ^ (((wn & 127) >> 4) << 5)) + (wn >> 7) * WG_IMG_BYTES;
      b_base[h] = (o ^ (((wm & 127) >> 4) << 5)) + (wm >> 7) * WG_IMG_BYTES +
                  OPB;
    }

    auto tr_read = [&](int off) {
      return __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
          (WG_LDS_AS mfma_bf16x4*)(lds_raw + off));
    };

    auto compute = [&](int bufoff) {
#pragma unroll
      for (int kh = 0; kh < 2; ++kh) {
        mfma_bf16x8 a[FN], b[FM];
        const int ko = bufoff + kh * 32 * 256;
#pragma unroll
        for (int i = 0; i < FN; ++i)
          a[i] = __builtin_shufflevector(
              tr_read((a_base[0] ^ (i << 5)) + ko),
              tr_read((a_base[1] ^ (i << 5)) + ko), 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
        for (int j = 0; j < FM; ++j)
          b[j] = __builtin_shufflevector(
              tr_read((b_base[0] ^ (j << 5)) + ko),
              tr_read((b_base[1] ^ (j << 5)) + ko), 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
        for (int i = 0; i < FN; ++i)
#pragma unroll
          for (int j = 0; j < FM; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a[i], b[j], acc[i][j], 0, 0, 0);
      }
    };

    // every wave drains its own DMAs, then the barrier publishes the
    // buffer: it is read only after a barrier that follows the wait, and
    // restaged only after the barrier that follows its last read
    auto publish = [] {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    };

    int cur = 0;
    stage(k_begin, cur);
    publish();
    for (int64_t k0 = k_begin + WG_BK; k0 < k_end; k0 += WG_BK) {
      stage(k0, cur ^ BUFB);
      compute(cur);
      publish();
      cur ^= BUFB;
    }
    compute(cur);
  } else {
    unsigned char* dyT = lds_raw;              // [TILE n][64 k] swizzled
    unsigned char* xT = lds_raw + TILE * 128;  // [TILE m][64 k]

    // staging map (per tile [64 k][TILE cols]): thread = 4 k-rows x 8 cols
    // (4 x 16 B coalesced loads -> 8 packed b64 transposed LDS writes)
    const int st_kg = (tid / SC) * 4;
    const int st_c = (tid % SC) * 8;

    const int a_row = lane & 15;
    const int a_k = (lane >> 4) * 8;
    const bool m_edge = (m0 + TILE) > M;
    const bool in0 = !m_edge || (m0 + st_c + 4) <= M;
    const bool in1 = !m_edge || (m0 + st_c + 8) <= M;

    // T14 split (guide G15): issue the NEXT step's global loads before this
    // step's MFMA phase so HBM latency hides under compute; the register
    // tile is written to LDS after the barrier.
    bf16x4 rdy[4][2], rx[4][2];

    auto load_step = [&](int64_t k0) {
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const unsigned short* src =
            dy + (k0 + st_kg + rr) * (int64_t)N + n0 + st_c;
        rdy[rr][0] = reinterpret_cast<const bf16x4*>(src)[0];
        rdy[rr][1] = reinterpret_cast<const bf16x4*>(src)[1];
        const unsigned short* srcx =
            x + (k0 + st_kg + rr) * (int64_t)M + m0 + st_c;
        // real branches (EXEC-masked loads): an out-of-range lane must not
        // issue the load at all (last row would read past the tensor)
        rx[rr][0] = bf16x4{0, 0, 0, 0};
        rx[rr][1] = bf16x4{0, 0, 0, 0};
        if (in0) rx[rr][0] = reinterpret_cast<const bf16x4*>(srcx)[0];
        if (in1) rx[rr][1] = reinterpret_cast<const bf16x4*>(srcx)[1];
      }
    };

    auto write_step = [&] {
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          U16x4 p{{rdy[0][h][j], rdy[1][h][j], rdy[2][h][j], rdy[3][h][j]}};
          *reinterpret_cast<unsigned long long*>(
              dyT + lds_off(st_c + h * 4 + j, st_kg)) = p.ll;
          U16x4 q{{rx[0][h][j], rx[1][h][j], rx[2][h][j], rx[3][h][j]}};
          *reinterpret_cast<unsigned long long*>(
              xT + lds_off(st_c + h * 4 + j, st_kg)) = q.ll;
        }
    };

    load_step(k_begin);
    for (int64_t k0 = k_begin; k0 < k_end; k0 += WG_BK) {
      write_step();
      __syncthreads();
      if (k0 + WG_BK < k_end)
        load_step(k0 + WG_BK);  // in flight under the MFMA phase
      // ---- MFMA: FN x FM fragments x 2 k-halves ---------------------------
#pragma unroll
      for (int kh = 0; kh < 2; ++kh) {
        mfma_bf16x8 a[FN], b[FM];
#pragma unroll
        for (int i = 0; i < FN; ++i)
          a[i] = *reinterpret_cast<const mfma_bf16x8*>(
              dyT + lds_off(wn + i * 16 + a_row, kh * 32 + a_k));
#pragma unroll
        for (int j = 0; j < FM; ++j)
          b[j] = *reinterpret_cast<const mfma_bf16x8*>(
              xT + lds_off(wm + j * 16 + a_row, kh * 32 + a_k));
#pragma unroll
        for (int i = 0; i < FN; ++i)
#pragma unroll
          for (int j = 0; j < FM; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a[i], b[j], acc[i][j], 0, 0, 0);
      }
      __syncthreads();
    }
  }

  // ---- epilogue: fp32 partial slab (column-masked) ----------------------
  float* out = part + (int64_t)blockIdx.x * N * M;
  const int c_col = lane & 15;
  const int c_row = (lane >> 4) * 4;
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FM; ++j) {
      const int col = m0 + wm + j * 16 + c_col;
      if (col >= M) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = n0 + wn + i * 16 + c_row + r;
        out[(int64_t)row * M + col] = acc[i][j][r];
      }
    }
}

// Which tile sizes take the LDS-DMA staging by default: the ones whose
// median beat the register staging's by more than the larger min..max
// spread at their bench shapes.  Both did (micro_gemm.py --wgrad-staging,
// profiles/r12_wgrad_glds.md): 256 at 1024x432 and 512x1024 by 14-25 us
// against spreads of 4-18, 128 at 256x512 by 7 us against 0.8.
template <int TILE>
constexpr bool kGldsDefault = TILE == 128 || TILE == 256;

template <int TILE>
torch::Tensor wgrad_launch(torch::Tensor dy, torch::Tensor x,
                           int64_t splitk, bool out_bf16,
                           c10::optional<bool> regstage) {
  TORCH_CHECK(dy.is_cuda() && dy.is_contiguous() && dy.dim() == 2 &&
              dy.scalar_type() == torch::kBFloat16,
              "dy must be [B, N] bf16 contiguous");
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 2 &&
              x.scalar_type() == torch::kBFloat16,
              "x must be [B, M] bf16 contiguous");
  const int64_t B = dy.size(0);
  const int N = static_cast<int>(dy.size(1));
  const int M = static_cast<int>(x.size(1));
  TORCH_CHECK(x.size(0) == B, "batch mismatch");
  TORCH_CHECK(N % TILE == 0 && M % 8 == 0 && B % WG_BK == 0,
              "wgrad_nt", TILE, " needs N % ", TILE,
              " == 0, M % 8 == 0, B % 64 == 0");
  const int tiles = (N / TILE) * ((M + TILE - 1) / TILE);
  // block budget of one full residency wave: 256 8-wave blocks (1 per CU,
  // 64 KB LDS) or 512 4-wave blocks.  sk sweep (scripts/micro_gemm.py):
  // >32 splits exceed it and cliff; 32 is the measured optimum
  constexpr int budget = TILE == 256 ? 256 : 512;
  if (splitk <= 0)
    splitk = std::min<int64_t>(
        32, std::max<int64_t>(1, budget / std::max(1, tiles)));
  // chunk must be a multiple of WG_BK covering B
  int64_t chunk = ((B + splitk - 1) / splitk + WG_BK - 1) / WG_BK * WG_BK;
  splitk = (B + chunk - 1) / chunk;
  auto part = torch::empty({splitk, N, M},
                           dy.options().dtype(torch::kFloat32));
  auto stream = c10::hip::getCurrentHIPStream().stream();
  dim3 grid(splitk, tiles);
  const bool glds = regstage.has_value() ? !*regstage : kGldsDefault<TILE>;
  auto kernel = glds ? wgrad_kernel<TILE, true> : wgrad_kernel<TILE, false>;
  hipLaunchKernelGGL(kernel, grid, dim3(2 * TILE), 0, stream,
                     reinterpret_cast<unsigned short*>(dy.data_ptr()),
                     reinterpret_cast<unsigned short*>(x.data_ptr()),
                     part.data_ptr<float>(), B, N, M, chunk);
  // fused split-K reduce (+bf16 cast when the consumer is a
  // bf16 parameter) — replaces torch reduce + .to elementwise
  return reduce_splitk(part, out_bf16);
}

}  // namespace

torch::Tensor wgrad_nt128(torch::Tensor dy, torch::Tensor x,
                          int64_t splitk, bool out_bf16,
                          c10::optional<bool> regstage) {
  return wgrad_launch<128>(dy, x, splitk, out_bf16, regstage);
}

torch::Tensor wgrad_nt256(torch::Tensor dy, torch::Tensor x,
                          int64_t splitk, bool out_bf16,
                          c10::optional<bool> regstage) {
  return wgrad_launch<256>(dy, x, splitk, out_bf16, regstage);
}

// Constants of the LDS-DMA staging and its image table, for the CPU
// mirror in tests/wgrad_image.py.
py::dict wgrad_glds_layout() {
  py::dict d;
  d["bk"] = WG_BK;
  d["img_cols"] = WG_IMG_COLS;
  d["img_bytes"] = WG_IMG_BYTES;
  d["fill_rows"] = WG_FILL_ROWS;
  d["fills_per_wave"] = WG_FILLS_PER_WAVE;
  d["buffers"] = 2;
  py::list off;
  for (int row = 0; row < WG_BK; ++row)
    for (int ch = 0; ch < 16; ++ch) off.append(lds_off_tr(row, ch));
  d["off"] = off;
  py::dict def;
  def[py::int_(128)] = kGldsDefault<128>;
  def[py::int_(256)] = kGldsDefault<256>;
  d["glds_default"] = def;
  return d;
}
