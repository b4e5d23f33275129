// The low-rank DCN-v2 cross layer  y = x0 * (U (V^T x) + b) + x  and its data
// gradient (docs/Kernels.md, "Low-rank cross layer", has the definition the
// kernel and the tests share).  One chained-GEMM template, two uses:
//
//   out[b, n] = epi( sum_j bf16_rne(sum_k A[b, k] * W1[j, k]) * W2[n, j] )
//
//   cross_lowrank_fwd:     A = x,  W1 = V [r, D],   W2 = U [D, r],
//                          epi = the cross epilogue (bias, x0, residual x),
//                          also writes t = bf16_rne(x V^T) and v when SAVE
//   cross_lowrank_bwd_dx:  A = dz, W1 = U^T [r, D], W2 = V^T [D, r],
//                          epi = + float(g), also writes dt
//
// Row band.  A block of four waves owns 128 rows and ALL D output columns;
// wave w owns rows 32 w .. 32 w + 31 in both phases, so the intermediate
// never crosses a wave.  A 1-D grid has one block per band (never capped:
// the block body in a band loop kept loop-invariant addresses live across
// both phases and spilled).
//
// Phase 1.  cross_fwd_kernel's k-loop over D in 64-wide steps
// (stage_kmajor_load/write, the next step's loads in flight under the
// MFMAs) into a [128][RP] tile, RP the rank padded to 32, 64 or 128 (a
// template parameter): W1 rows >= r are zero in the LDS image, never in
// memory.  A is read once per band.
//
// Hand-over, in registers.  The W1 fragment is the MFMA's first operand, so
// accumulator register e of lane l in fragment (i, j) is
// t32[row 16 i + l % 16][rank 16 j + 4 (l / 16) + e]: the lane already owns
// the ROW the second GEMM's operand fragment wants from it (l % 16), and a
// contraction index may be permuted if both operands agree.  Fragments 2 s
// and 2 s + 1, rounded once, are phase 2's operand for its k-step s with
// MFMA k position 8 q + e (q = l / 16) meaning
//   rank 32 s + 16 (e / 4) + 4 q + e % 4,
// and the W2 fragment is read from LDS as two 8-byte halves at exactly those
// ranks.  No LDS image of t, no barrier, and the 8-byte stores of t / dt to
// memory come from the same registers: what is stored is what phase 2 eats.
//
// Phase 2.  64-column tiles of the output: the tile's W2 [64][RP] slab is
// register-staged into LDS in one load step (thread t: row t / 4, ranks
// 32 (t % 4) ..; rows >= D and ranks >= r zero), the next tile's slab loads
// are in flight under this tile's MFMAs and epilogue.  Epilogue:
// cross_fwd_kernel's, the tile's fp32 accumulators parked in its
// XOR-swizzled half-tile image (32 KB: the same LDS the slab and phase 1
// use), all threads walking it in the row/oct map with 16-byte loads and
// stores.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <tuple>
#include "mfma_tile.h"

bool cross_rows_ok(torch::Tensor t);

namespace {

// the fp32 epilogue arithmetic stays scalar instructions
#define CLR_KERNEL __attribute__((target("no-packed-fp32-ops")))

#define CLR_BK 64
#define CLR_BAND 128
#define CLR_PW 64      // columns per phase-2 tile
#define CLR_IMG 16384  // one [128][64 k] bf16 image
#define CLR_CHUNK 8192  // one [64 n][64 j] chunk of the W2 slab
#define CLR_MIN_D 16
#define CLR_MAX_D 1024
#define CLR_MIN_R 16
#define CLR_MAX_R 128

// __syncthreads(), spelled out (cross_layer.hip has the reason)
__device__ __forceinline__ void block_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// cross_fwd_kernel's parked half tile: fp32 [row][col], 256 B rows, the
// 16 B chunk index XOR the row
__device__ __forceinline__ int park_off32(int row, int col) {
  return row * 256 + ((((col >> 2) ^ row) & 15) << 4) + (col & 3) * 4;
}

// one operand fragment, as the MFMA takes it and as its two rank quads
union Frag {
  mfma_bf16x8 b;
  bf16x4 h[2];
  unsigned long long q[2];
};

// CROSS: out = x0 * (acc + bias) + res (res = A = x), V = bf16(acc + bias)
// and T when SAVE.  !CROSS: out = acc + res (res = g), T always.
template <int RP, bool CROSS, bool SAVE>
__global__ CLR_KERNEL __launch_bounds__(2 * CLR_BAND, 2)
void cross_lowrank_chain_kernel(const unsigned short* A, int64_t lda,
                                const unsigned short* __restrict__ W1,
                                const unsigned short* __restrict__ W2,
                                const unsigned short* RES, int64_t ldr,
                                const unsigned short* __restrict__ X0,
                                int64_t ld0,
                                const unsigned short* __restrict__ bias,
                                unsigned short* __restrict__ OUT,
                                unsigned short* __restrict__ V,
                                unsigned short* __restrict__ T,
                                int64_t M, int D, int r) {
  constexpr int FI = 2;                  // 32 rows per wave
  constexpr int FJ1 = RP / 16;           // phase 1: all of the padded rank
  constexpr int FJ2 = CLR_PW / 16;       // phase 2: 64 columns
  constexpr int KS = RP / 32;            // phase 2 k-steps
  constexpr int OPR = CLR_PW / 8;        // octs per parked row
  constexpr int RPS = 2 * CLR_BAND / OPR;  // rows per walk sweep
  constexpr int SW = CLR_BAND / RPS;     // sweeps per half
  constexpr bool SAVE_T = SAVE || !CROSS;

  __shared__ __attribute__((aligned(16))) unsigned char lds_raw[2 * CLR_IMG];
  unsigned char* xT = lds_raw;            // phase 1: [128 m][64 k]
  unsigned char* wT = lds_raw + CLR_IMG;  // phase 1: [RP j][64 k]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wm = (tid >> 6) * 32;
  const int st_r = tid >> 1;
  const int st_k = (tid & 1) * 32;
  const int sl_r = tid >> 2;  // the W2 slab: 64 rows x up to 128 ranks
  const int sl_k = (tid & 3) * 32;
  int f_col, f_row4;
  frag_pos(lane, f_col, f_row4);
  const int w_row = tid / OPR;
  const int w_oct = tid - w_row * OPR;

  {  // one band per block: the grid is never capped (host check)
    const int64_t m0 = (int64_t)blockIdx.x * CLR_BAND;
    const bool a_row_ok = (m0 + st_r) < M;  // ragged band
    const bool w1_row_ok = st_r < r;        // rank padding: zero rows

    // ---- phase 1: t32 [128][RP] = A[band] @ W1^T -------------------------
    mfma_f32x4 acc1[FI][FJ1];
    zero_acc(acc1);
    bf16x8 rx[4], rw[4];
    // the lambdas carry the kernel's target attribute, or they are not
    // inlined
    auto load_step = [&](int k0) CLR_KERNEL {
      stage_kmajor_load(rx, A + (m0 + st_r) * lda + k0 + st_k, a_row_ok,
                        k0 + st_k, D);
      stage_kmajor_load(rw, W1 + (int64_t)st_r * D + k0 + st_k, w1_row_ok,
                        k0 + st_k, D);
    };
    load_step(0);
    for (int k0 = 0; k0 < D; k0 += CLR_BK) {
      stage_kmajor_write(xT, rx, st_r, st_k);
      if (st_r < RP) stage_kmajor_write(wT, rw, st_r, st_k);
      block_sync();
      if (k0 + CLR_BK < D) load_step(k0 + CLR_BK);  // in flight under MFMA
      // the W1 fragment goes first (header comment)
      mfma_kstep<FI, FJ1, lds_off_linear, lds_off_linear, true>(
          acc1, xT, wT, wm, 0, lane);
      block_sync();
    }

    // the first W2 slab, in flight under the hand-over
    bf16x8 rs[4];
    auto load_slab = [&](int n0) CLR_KERNEL {
      stage_kmajor_load(rs, W2 + (int64_t)(n0 + sl_r) * r + sl_k,
                        sl_k < RP && (n0 + sl_r) < D, sl_k, r);
    };
    load_slab(0);

    // ---- hand-over: round once, keep as phase 2's operand, store t -------
    Frag tb[FI][KS];
#pragma unroll
    for (int i = 0; i < FI; ++i)
#pragma unroll
      for (int s = 0; s < KS; ++s) {
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int e = 0; e < 4; ++e)
            tb[i][s].h[h][e] = f32_to_bf16(acc1[i][2 * s + h][e]);
        if (SAVE_T) {
          const int64_t row = m0 + wm + i * 16 + f_col;
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int j = 32 * s + 16 * h + f_row4;  // r % 16 == 0
            if (row < M && j < r)
              *reinterpret_cast<bf16x4*>(T + row * r + j) = tb[i][s].h[h];
          }
        }
      }

    // ---- phase 2: out[band][n0 ..] = epi(t @ W2[n0 ..]^T) ---------------
    for (int n0 = 0; n0 < D; n0 += CLR_PW) {
      if (sl_k < RP)
        stage_kmajor_write(lds_raw + (sl_k >> 6) * CLR_CHUNK, rs, sl_r,
                           sl_k & 63);
      block_sync();
      if (n0 + CLR_PW < D) load_slab(n0 + CLR_PW);  // under this tile

      mfma_f32x4 acc[FI][FJ2];
      zero_acc(acc);
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const unsigned char* img = lds_raw + (s >> 1) * CLR_CHUNK;
        const int kb = (s & 1) * 32 + f_row4;  // the permuted ranks
        Frag wf[FJ2];
#pragma unroll
        for (int j = 0; j < FJ2; ++j) {
          wf[j].q[0] = *reinterpret_cast<const unsigned long long*>(
              img + lds_off_linear(j * 16 + f_col, kb));
          wf[j].q[1] = *reinterpret_cast<const unsigned long long*>(
              img + lds_off_linear(j * 16 + f_col, kb + 16));
        }
#pragma unroll
        for (int i = 0; i < FI; ++i)
#pragma unroll
          for (int j = 0; j < FJ2; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                wf[j].b, tb[i][s].b, acc[i][j], 0, 0, 0);
      }

      // epilogue operands, in flight under the park
      const int col = n0 + w_oct * 8;
      const bool col_ok = col < D;  // D % 16 == 0: whole octs
      bf16x8 x0v[SW], resv[SW];
      bf16x8 bv = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (CROSS && col_ok) bv = *reinterpret_cast<const bf16x8*>(bias + col);
#pragma unroll
      for (int s = 0; s < SW; ++s) {
        const int64_t row = m0 + s * RPS + w_row;
        x0v[s] = resv[s] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if (col_ok && row < M) {
          if (CROSS)
            x0v[s] = *reinterpret_cast<const bf16x8*>(X0 + row * ld0 + col);
          resv[s] = *reinterpret_cast<const bf16x8*>(RES + row * ldr + col);
        }
      }
      block_sync();  // the slab is free: the park takes its place
      // fragment (i, j): row wm + i*16 + f_col, columns n0 + j*16 + f_row4
      // + 0..3
#pragma unroll
      for (int i = 0; i < FI; ++i)
#pragma unroll
        for (int j = 0; j < FJ2; ++j)
          *reinterpret_cast<f32x4*>(
              lds_raw + park_off32(wm + i * 16 + f_col, j * 16 + f_row4)) =
              f32x4{acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
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
          const float a32 = j < 4 ? lo[j & 3] : hi[j & 3];
          const float res = bf16_to_f32(resv[s][j]);
          if (CROSS) {
            const float v32 = a32 + bf16_to_f32(bv[j]);
            yo[j] = f32_to_bf16(bf16_to_f32(x0v[s][j]) * v32 + res);
            if (SAVE) vo[j] = f32_to_bf16(v32);
          } else {
            yo[j] = f32_to_bf16(a32 + res);
          }
        }
        if (col_ok && row < M) {
          *reinterpret_cast<bf16x8*>(OUT + row * D + col) = yo;
          if (CROSS && SAVE)
            *reinterpret_cast<bf16x8*>(V + row * D + col) = vo;
        }
      }
      block_sync();
    }
  }
}

int64_t row_ld(const torch::Tensor& t) {
  return t.size(0) > 1 ? t.stride(0) : t.size(1);
}

bool dim_ok(int64_t d) {
  return d % 16 == 0 && d >= CLR_MIN_D && d <= CLR_MAX_D;
}

// one block per band
bool bands_ok(int64_t rows) {
  return (rows + CLR_BAND - 1) / CLR_BAND < (1LL << 31);
}

bool rank_ok(int64_t r) {
  return r % 16 == 0 && r >= CLR_MIN_R && r <= CLR_MAX_R;
}

// contiguous bf16 [rows, cols] on the GPU with a 16 B aligned base
bool weight_ok(const torch::Tensor& w, int64_t rows, int64_t cols) {
  return w.is_cuda() && w.scalar_type() == torch::kBFloat16 && w.dim() == 2 &&
         w.size(0) == rows && w.size(1) == cols && w.is_contiguous() &&
         miyarn_aligned(w.data_ptr(), 16);
}

const unsigned short* cptr(const torch::Tensor& t) {
  return reinterpret_cast<const unsigned short*>(t.data_ptr());
}
unsigned short* mptr(torch::Tensor& t) {
  return reinterpret_cast<unsigned short*>(t.data_ptr());
}

template <bool CROSS, bool SAVE>
void launch_chain(const torch::Tensor& a, const torch::Tensor& w1,
                  const torch::Tensor& w2, const torch::Tensor& res,
                  const unsigned short* x0, int64_t ld0,
                  const unsigned short* bias, unsigned short* out,
                  unsigned short* v, unsigned short* t, int r) {
  const int64_t M = a.size(0);
  const int D = static_cast<int>(a.size(1));
  const dim3 grid(static_cast<unsigned>((M + CLR_BAND - 1) / CLR_BAND));
  auto stream = c10::hip::getCurrentHIPStream().stream();
  auto* kern = r <= 32   ? cross_lowrank_chain_kernel<32, CROSS, SAVE>
               : r <= 64 ? cross_lowrank_chain_kernel<64, CROSS, SAVE>
                         : cross_lowrank_chain_kernel<128, CROSS, SAVE>;
  hipLaunchKernelGGL(kern, grid, dim3(2 * CLR_BAND), 0, stream, cptr(a),
                     row_ld(a), cptr(w1), cptr(w2), cptr(res), row_ld(res),
                     x0, ld0, bias, out, v, t, M, D, r);
}

}  // namespace

bool cross_lowrank_ok(torch::Tensor x0, torch::Tensor x,
                      torch::Tensor v_weight, torch::Tensor u_weight,
                      torch::Tensor bias) {
  if (!(cross_rows_ok(x0) && cross_rows_ok(x) && x0.sizes() == x.sizes() &&
        v_weight.dim() == 2))
    return false;
  const int64_t D = x.size(1);
  const int64_t r = v_weight.size(0);
  return dim_ok(D) && rank_ok(r) && weight_ok(v_weight, r, D) &&
         weight_ok(u_weight, D, r) && bias.is_cuda() &&
         bias.scalar_type() == torch::kBFloat16 && bias.dim() == 1 &&
         bias.size(0) == D && bias.is_contiguous() &&
         miyarn_aligned(bias.data_ptr(), 16) && x0.device() == x.device() &&
         x.device() == v_weight.device() &&
         x.device() == u_weight.device() && x.device() == bias.device() &&
         bands_ok(x.size(0));
}

std::tuple<torch::Tensor, c10::optional<torch::Tensor>,
           c10::optional<torch::Tensor>>
cross_lowrank_fwd(torch::Tensor x0, torch::Tensor x, torch::Tensor v_weight,
                  torch::Tensor u_weight, torch::Tensor bias, bool save) {
  TORCH_CHECK(cross_lowrank_ok(x0, x, v_weight, u_weight, bias),
              "cross_lowrank_fwd needs bf16 x0, x [B, D] (unit column "
              "stride, row stride % 8 == 0, 16 B aligned), v_weight [r, D], "
              "u_weight [D, r] and bias [D] contiguous on one GPU, "
              "D % 16 == 0, 16 <= D <= 1024, r % 16 == 0, 16 <= r <= 128");
  const int64_t M = x.size(0);
  const int64_t D = x.size(1);
  const int r = static_cast<int>(v_weight.size(0));
  auto y = torch::empty({M, D}, x.options());
  c10::optional<torch::Tensor> t, v;
  if (save) {
    t = torch::empty({M, (int64_t)r}, x.options());
    v = torch::empty({M, D}, x.options());
  }
  if (M == 0) return {y, t, v};
  if (save)
    launch_chain<true, true>(x, v_weight, u_weight, x, cptr(x0), row_ld(x0),
                             cptr(bias), mptr(y), mptr(*v), mptr(*t), r);
  else
    launch_chain<true, false>(x, v_weight, u_weight, x, cptr(x0), row_ld(x0),
                              cptr(bias), mptr(y), nullptr, nullptr, r);
  return {y, t, v};
}

// (dx, dt) with dt = bf16(dz @ U) and dx = bf16(dt @ V + g); ut = U^T [r, D]
// and vt = V^T [D, r] are contiguous copies the caller makes.
std::vector<torch::Tensor> cross_lowrank_bwd_dx(torch::Tensor dz,
                                                torch::Tensor g,
                                                torch::Tensor ut,
                                                torch::Tensor vt) {
  TORCH_CHECK(cross_rows_ok(dz) && cross_rows_ok(g) &&
              dz.sizes() == g.sizes() && dim_ok(dz.size(1)) &&
              bands_ok(dz.size(0)) &&
              ut.dim() == 2 && rank_ok(ut.size(0)) &&
              weight_ok(ut, ut.size(0), dz.size(1)) &&
              weight_ok(vt, dz.size(1), ut.size(0)) &&
              dz.device() == g.device() && dz.device() == ut.device() &&
              dz.device() == vt.device(),
              "cross_lowrank_bwd_dx needs bf16 dz, g [B, D] (unit column "
              "stride, row stride % 8 == 0, 16 B aligned), ut [r, D] and "
              "vt [D, r] contiguous on one GPU, D % 16 == 0, "
              "16 <= D <= 1024, r % 16 == 0, 16 <= r <= 128");
  const int64_t M = dz.size(0);
  const int64_t D = dz.size(1);
  const int r = static_cast<int>(ut.size(0));
  auto dx = torch::empty({M, D}, dz.options());
  auto dt = torch::empty({M, (int64_t)r}, dz.options());
  if (M == 0) return {dx, dt};
  launch_chain<false, true>(dz, ut, vt, g, nullptr, 0, nullptr, mptr(dx),
                            nullptr, mptr(dt), r);
  return {dx, dt};
}
