// Fused multi-table embedding lookup + sparse-gradient apply for MI355X.
//
// The dominant cost of Criteo CTR models (SURVEY §7 "hard parts": sparse
// embedding gradient reduce).  All categorical tables are concatenated into
// one [total_rows, D] fp32 buffer; Python pre-adds per-feature row offsets
// into the flat id tensor, so the kernels are pure row gather / row
// scatter (the single-GPU step's emb_lookup_fused and the fused SGD
// scatter take the raw ids and add the offsets themselves):
//
//  * emb_fwd:      out[i, :] = table[ids[i], :]          (out fp32 or bf16;
//                  bf16 out fuses the mixed-precision cast into the gather)
//  * emb_bwd_sgd:  table[ids[i], :] -= lr * scale * g[i, :]   (fused
//                  backward+update, atomicAdd fp32 — no materialized
//                  dense gradient table)
//  * emb_bwd_dense: grad_table[ids[i], :] += scale * g[i, :]  (for
//                  optimizers that need the dense gradient)
//
// Row layout keeps consecutive d contiguous.  The gathers give a lane a
// quad of a row (16 B loads; reuse across the batch is served by L2/LLC,
// guide Appendix B "Scatter/gather/embedding").  The atomic scatters give
// a lane ONE float, so that a wave-instruction adds whole contiguous row
// segments: they are bound by the number of 64-byte atomic requests, not
// by bytes (see "atomic scatter: the row-segment map" below).

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include "common.h"
#include <cstdlib>

namespace {

template <typename OIo>
__global__ void emb_fwd_kernel(const float* __restrict__ table,
                               const int64_t* __restrict__ ids,
                               typename OIo::scalar_t* __restrict__ out,
                               int64_t n_rows, int64_t dim) {
  const int64_t dvec = dim >> 2;
  const int64_t total = n_rows * dvec;
  const int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
       t < total; t += stride) {
    const int64_t row = t / dvec;
    const int64_t c4 = t - row * dvec;
    const int64_t src = ids[row];
    f32x4 v = reinterpret_cast<const f32x4*>(table + src * dim)[c4];
    float vv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) vv[j] = v[j];
    QuadIo<OIo>::store4(out, row * dvec + c4, vv);
  }
}

// ---- atomic scatter: the row-segment map ----------------------------------
//
// Float atomics execute at the memory side: a wave-instruction leaves L2
// as one uncached request per 64-byte line it touches, and the chip
// retires a fixed number of such requests per second (docs/Kernels.md,
// "Embedding", has the model and the measurements).  So the map gives one
// lane ONE FLOAT and `dim` consecutive lanes one update row: at dim 16 a
// wave-instruction adds four whole 64-byte rows (4 requests), where a
// quad-per-thread map touches 16 rows in four instructions of 16 requests
// each - 4 requests per row instead of 1.  Rows wider than 64 floats span
// consecutive instructions of 256 contiguous bytes; a dim that does not
// divide 64 lets a row straddle two waves, which is correct and merely
// costs that row one more request.
//
// One element per thread per grid-stride trip: at the bench shape more
// elements per trip, a wider grid and a once-per-row id read broadcast by
// a wave shuffle all measured within 3% of this, the atomics being the
// only cost that shows (16 lanes reading one id are a single 8-byte
// request).  DIM = 16 is the flagship instantiation (shifts); DIM = 0
// reads the runtime dim, pays an int64 divide per element and serves
// every other dim, dims that are no multiple of 4 included.  With WIDE,
// the lane holding float 0 of a row also adds the wide (dim-1) table's
// scalar: exactly once per update row.  With STRIDED the gradient is a
// row-strided [batch, g_div * dim] view (a column slice of the MLP-input
// gradient, read where backward left it): batch row b starts g_pad
// elements later than it would in a dense array, per row before it.
// With OFFS, `ids` is the raw [batch, g_div] array of per-feature ids and
// the kernel adds offsets[row % g_div] itself, so no pre-added copy of the
// ids has to exist; the other instantiations never look at `offsets`.
template <typename GIo, int DIM, bool WIDE, bool STRIDED, bool OFFS = false>
__device__ __forceinline__ void scatter_row_segments(
    float* __restrict__ table, float* __restrict__ wide_table,
    const int64_t* __restrict__ ids,
    const typename GIo::scalar_t* __restrict__ g,
    const typename GIo::scalar_t* __restrict__ gw,
    int64_t n_rows, int64_t dim_rt, int g_div, int64_t g_pad,
    float alpha, float wide_alpha,
    const int64_t* __restrict__ offsets = nullptr) {
  const int64_t dim = DIM ? DIM : dim_rt;
  const int64_t total = n_rows * dim;
  const int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
       t < total; t += stride) {
    const int64_t row = t / dim;  // a shift when DIM is a power of two
    const int64_t c = t - row * dim;
    int64_t id = ids[row];
    if (OFFS) id += offsets[row - (row / g_div) * g_div];
    const int64_t gi = STRIDED ? t + (row / g_div) * g_pad : t;
    f32_atomic_add(table + id * dim + c, alpha * GIo::load(g, gi));
    if (WIDE && c == 0)
      f32_atomic_add(wide_table + id,
                     wide_alpha * GIo::load(gw, row / g_div));
  }
}

template <typename GIo, int DIM>
__global__ void emb_bwd_sgd_kernel(float* __restrict__ table,
                                   const int64_t* __restrict__ ids,
                                   const typename GIo::scalar_t* __restrict__ g,
                                   int64_t n_rows, int64_t dim,
                                   float neg_lr_scale) {
  scatter_row_segments<GIo, DIM, false, false>(
      table, nullptr, ids, g, nullptr, n_rows, dim, 1, 0, neg_lr_scale,
      0.f);
}

template <typename GIo, int DIM>
__global__ void emb_bwd_dense_kernel(
    float* __restrict__ grad_table,
    const int64_t* __restrict__ ids,
    const typename GIo::scalar_t* __restrict__ g,
    int64_t n_rows, int64_t dim, float scale) {
  scatter_row_segments<GIo, DIM, false, false>(
      grad_table, nullptr, ids, g, nullptr, n_rows, dim, 1, 0, scale, 0.f);
}

// Fused deep+wide sparse update: the CTR models' wide (dim-1) table is
// driven by the SAME flat ids as the deep (dim-16) table, so one kernel
// reads the ids once and issues both updates (separate kernels re-read
// 13.6 MB of ids and pay an extra launch).
template <typename GIo, int DIM, bool STRIDED>
__global__ void emb_bwd_sgd_fused_wide_kernel(
    float* __restrict__ table, float* __restrict__ wide_table,
    const int64_t* __restrict__ ids,
    const typename GIo::scalar_t* __restrict__ g,
    const typename GIo::scalar_t* __restrict__ gw,
    int64_t n_rows, int64_t dim, int g_div, int64_t g_pad,
    float neg_lr_scale, float wide_alpha) {
  scatter_row_segments<GIo, DIM, true, STRIDED>(
      table, wide_table, ids, g, gw, n_rows, dim, g_div, g_pad,
      neg_lr_scale, wide_alpha);
}

// The same update from the raw [batch, g_div] ids: offsets[f] is added in
// the kernel, so the single-GPU step never writes (forward) nor re-reads
// (here) a 13.6 MB pre-added copy of the ids.
template <typename GIo, int DIM, bool STRIDED>
__global__ void emb_bwd_sgd_fused_wide_offs_kernel(
    float* __restrict__ table, float* __restrict__ wide_table,
    const int64_t* __restrict__ ids, const int64_t* __restrict__ offsets,
    const typename GIo::scalar_t* __restrict__ g,
    const typename GIo::scalar_t* __restrict__ gw,
    int64_t n_rows, int64_t dim, int g_div, int64_t g_pad,
    float neg_lr_scale, float wide_alpha) {
  scatter_row_segments<GIo, DIM, true, STRIDED, true>(
      table, wide_table, ids, g, gw, n_rows, dim, g_div, g_pad,
      neg_lr_scale, wide_alpha, offsets);
}

// Scalar gather for dim % 4 != 0 (e.g. the wide part's dim-1 tables).
template <typename OIo>
__global__ void emb_fwd_scalar_kernel(const float* __restrict__ table,
                                      const int64_t* __restrict__ ids,
                                      typename OIo::scalar_t* __restrict__ out,
                                      int64_t n_rows, int64_t dim) {
  const int64_t total = n_rows * dim;
  const int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
       t < total; t += stride) {
    const int64_t row = t / dim;
    const int64_t c = t - row * dim;
    OIo::store(out, t, table[ids[row] * dim + c]);
  }
}

// Wide-part fusion: out[b] = sum_f table[ids[b*F + f]] for scalar
// (dim-1) tables — replaces gather + torch reduce with one kernel.
template <typename OIo>
__global__ void emb_gather_sum_kernel(const float* __restrict__ table,
                                      const int64_t* __restrict__ ids,
                                      typename OIo::scalar_t* __restrict__ out,
                                      int64_t batch, int F) {
  const int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
       b < batch; b += stride) {
    float acc = 0.f;
    const int64_t* row = ids + b * F;
#pragma unroll 4
    for (int f = 0; f < F; ++f) acc += table[row[f]];
    OIo::store(out, b, acc);
  }
}

// Backward of gather-sum: table[ids[b*F+f]] += alpha * g[b]
template <typename GIo>
__global__ void emb_scatter_sum_kernel(float* __restrict__ table,
                                       const int64_t* __restrict__ ids,
                                       const typename GIo::scalar_t* __restrict__ g,
                                       int64_t batch, int F, float alpha) {
  const int64_t total = batch * (int64_t)F;
  const int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
       t < total; t += stride) {
    const int64_t b = t / F;
    f32_atomic_add(table + ids[t], alpha * GIo::load(g, b));
  }
}

// Gather straight into a slice of the MLP input buffer: gather row
// (b, f) = ids[b*F + f] lands at out[b, col_off + f*dim : ...], killing
// the separate concat kernel (out stride/offset in quads; host guarantees
// dim % 4 == 0 and col_off % 4 == 0).
template <typename OIo>
__global__ void emb_fwd_into_kernel(const float* __restrict__ table,
                                    const int64_t* __restrict__ ids,
                                    typename OIo::scalar_t* __restrict__ out,
                                    int64_t n_rows, int64_t dim, int F,
                                    int64_t out_stride_q, int64_t off_q) {
  const int64_t dvec = dim >> 2;
  const int64_t total = n_rows * dvec;
  const int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
       t < total; t += stride) {
    const int64_t row = t / dvec;
    const int64_t c4 = t - row * dvec;
    const int64_t b = row / F;
    const int64_t f = row - b * F;
    f32x4 v = reinterpret_cast<const f32x4*>(table + ids[row] * dim)[c4];
    float vv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) vv[j] = v[j];
    QuadIo<OIo>::store4(out, b * out_stride_q + off_q + f * dvec + c4,
                        vv);
  }
}

// The whole single-GPU sparse forward in one pass over the raw ids: the
// per-feature offset add, the deep gather into the MLP-input slice
// (emb_fwd_into_kernel's cast and layout), the wide gather-sum, and the
// dense / zero-pad columns in front of the slice.  Separately these were
// a torch int64 add that wrote a 13.6 MB flat-id array, two kernels that
// each read it back, and two small torch fills.
//
// A block owns chunks of `rows_per_chunk` whole batch rows and walks a
// chunk's output quads in row-major order, so a row of `out` is written
// front to back by consecutive lanes.  The lane that holds quad 0 of
// (b, f) also loads the wide scalar of that id and parks it in LDS; after
// the barrier ONE thread per batch row adds its F scalars in the order
// f = 0 .. F-1 from 0.f, which is emb_gather_sum_kernel's sum to the bit
// (a tree or shuffle reduction would not be).
#define LOOKUP_ROWS 32          // batch rows of a chunk
#define LOOKUP_LDS_FLOATS 2048  // parked wide scalars: rows_per_chunk * F

template <typename OIo>
__global__ void emb_lookup_fused_kernel(
    const float* __restrict__ table, const float* __restrict__ wide_table,
    const int64_t* __restrict__ ids, const int64_t* __restrict__ offsets,
    const typename OIo::scalar_t* __restrict__ dense,
    typename OIo::scalar_t* __restrict__ out,
    typename OIo::scalar_t* __restrict__ wide_out,
    int64_t batch, int dim, int F, int rows_per_chunk,
    int64_t out_stride_q, int off_q, int n_dense) {
  __shared__ float wide_s[LOOKUP_LDS_FLOATS];
  const int dvec = dim >> 2;
  const int ipr = off_q + F * dvec;  // quads written per batch row
  const int64_t n_chunks = (batch + rows_per_chunk - 1) / rows_per_chunk;
  for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
    const int64_t b0 = chunk * rows_per_chunk;
    const int nr = (int)min((int64_t)rows_per_chunk, batch - b0);
    const int items = nr * ipr;
    for (int t = threadIdx.x; t < items; t += blockDim.x) {
      const int r = t / ipr;
      const int i = t - r * ipr;
      const int64_t b = b0 + r;
      float vv[4];
      if (i < off_q) {
        // dense features, then zeros up to the slice (bf16 -> f32 -> bf16
        // returns the stored bits)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int col = i * 4 + j;
          vv[j] = col < n_dense
                      ? OIo::load(dense, b * (int64_t)n_dense + col)
                      : 0.f;
        }
      } else {
        const int gq = i - off_q;
        const int f = gq / dvec;
        const int c4 = gq - f * dvec;
        const int64_t id = ids[b * F + f] + offsets[f];
        f32x4 v = reinterpret_cast<const f32x4*>(table + id * dim)[c4];
        if (c4 == 0) wide_s[r * F + f] = wide_table[id];
#pragma unroll
        for (int j = 0; j < 4; ++j) vv[j] = v[j];
      }
      QuadIo<OIo>::store4(out, b * out_stride_q + i, vv);
    }
    __syncthreads();
    for (int r = threadIdx.x; r < nr; r += blockDim.x) {
      float acc = 0.f;
      const float* row = wide_s + r * F;
#pragma unroll 4
      for (int f = 0; f < F; ++f) acc += row[f];
      OIo::store(wide_out, b0 + r, acc);
    }
    __syncthreads();  // the next chunk overwrites wide_s
  }
}

// Sorted segmented scatter+SGD: ids are SORTED so duplicates are
// contiguous; only the head thread of each run applies the (summed)
// update with a plain read-modify-write — no atomics (measured 4.6x
// faster than atomicAdd at the bench shape; see scripts/micro_scatter).
template <typename GIo>
__global__ void emb_bwd_sgd_sorted_kernel(
    float* __restrict__ table, const int64_t* __restrict__ ids,
    const typename GIo::scalar_t* __restrict__ g,
    int64_t n_rows, int64_t dim, float neg_lr_scale) {
  const int64_t dvec = dim >> 2;
  const int64_t total = n_rows * dvec;
  const int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
       t < total; t += stride) {
    const int64_t row = t / dvec;
    const int64_t c4 = t - row * dvec;
    const int64_t id = ids[row];
    if (row > 0 && ids[row - 1] == id) continue;  // not a run head
    float acc[4];
    QuadIo<GIo>::load4(g, row * dvec + c4, acc);
    for (int64_t r = row + 1; r < n_rows && ids[r] == id; ++r) {
      float more[4];
      QuadIo<GIo>::load4(g, r * dvec + c4, more);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] += more[j];
    }
    float* dst = table + id * dim + c4 * 4;
    f32x4 cur = *reinterpret_cast<f32x4*>(dst);
#pragma unroll
    for (int j = 0; j < 4; ++j) cur[j] += neg_lr_scale * acc[j];
    *reinterpret_cast<f32x4*>(dst) = cur;
  }
}

// Out-of-range ids silently corrupt adjacent table rows via atomicAdd;
// MIYARN_DEBUG_BOUNDS=1 turns on a host-side min/max validation (two
// small reductions + sync per call — debug only, off in production).
bool bounds_debug_enabled() {
  static const bool on = [] {
    const char* v = std::getenv("MIYARN_DEBUG_BOUNDS");
    return v != nullptr && v[0] != '\0' && v[0] != '0';
  }();
  return on;
}

void debug_check_ids(const torch::Tensor& ids, int64_t rows) {
  if (!bounds_debug_enabled() || ids.numel() == 0) return;
  const int64_t mn = ids.min().item<int64_t>();
  const int64_t mx = ids.max().item<int64_t>();
  TORCH_CHECK(mn >= 0 && mx < rows, "embedding ids out of range: [", mn,
              ", ", mx, "] vs table rows ", rows,
              " (MIYARN_DEBUG_BOUNDS check)");
}

void check_emb(const torch::Tensor& table, const torch::Tensor& ids,
               int64_t dim) {
  TORCH_CHECK(table.is_cuda() && table.is_contiguous() &&
              table.scalar_type() == torch::kFloat32,
              "table must be a contiguous fp32 GPU tensor");
  TORCH_CHECK(ids.is_cuda() && ids.is_contiguous() &&
              ids.scalar_type() == torch::kInt64,
              "ids must be contiguous int64 on GPU");
}

// Launch a row-segment scatter kernel: k16 is its dim-16 instantiation,
// k0 the runtime-dim one.  Atomic latency is higher than load latency, so
// the cap is 4x the streaming kernels'; the time is flat from 2048 blocks
// to an uncapped grid (docs/Kernels.md).
template <typename K16, typename K0, typename... Args>
void launch_row_segments(K16 k16, K0 k0, int64_t n, int64_t dim,
                         hipStream_t stream, Args... args) {
  const int grid = miyarn_grid_cap(n * dim, 8192);
  if (dim == 16)
    hipLaunchKernelGGL(k16, dim3(grid), dim3(MIYARN_BLOCK), 0, stream,
                       args...);
  else
    hipLaunchKernelGGL(k0, dim3(grid), dim3(MIYARN_BLOCK), 0, stream,
                       args...);
}

}  // namespace

torch::Tensor emb_fwd(torch::Tensor table, torch::Tensor ids,
                      bool out_bf16) {
  const int64_t dim = table.size(1);
  const int64_t n = ids.numel();
  check_emb(table, ids, dim);
  debug_check_ids(ids, table.size(0));
  auto out = torch::empty(
      {n, dim}, table.options().dtype(
          out_bf16 ? torch::kBFloat16 : torch::kFloat32));
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const bool vec = (dim % 4 == 0);
  int grid = miyarn_grid(n * (vec ? dim / 4 : dim));
  if (out_bf16) {
    auto* optr = reinterpret_cast<unsigned short*>(out.data_ptr());
    if (vec)
      hipLaunchKernelGGL(emb_fwd_kernel<Bf16Io>, dim3(grid),
                         dim3(MIYARN_BLOCK), 0, stream,
                         table.data_ptr<float>(), ids.data_ptr<int64_t>(),
                         optr, n, dim);
    else
      hipLaunchKernelGGL(emb_fwd_scalar_kernel<Bf16Io>, dim3(grid),
                         dim3(MIYARN_BLOCK), 0, stream,
                         table.data_ptr<float>(), ids.data_ptr<int64_t>(),
                         optr, n, dim);
  } else {
    if (vec)
      hipLaunchKernelGGL(emb_fwd_kernel<F32Io>, dim3(grid),
                         dim3(MIYARN_BLOCK), 0, stream,
                         table.data_ptr<float>(), ids.data_ptr<int64_t>(),
                         out.data_ptr<float>(), n, dim);
    else
      hipLaunchKernelGGL(emb_fwd_scalar_kernel<F32Io>, dim3(grid),
                         dim3(MIYARN_BLOCK), 0, stream,
                         table.data_ptr<float>(), ids.data_ptr<int64_t>(),
                         out.data_ptr<float>(), n, dim);
  }
  return out;
}

void emb_bwd_sgd(torch::Tensor table, torch::Tensor ids, torch::Tensor grad,
                 double lr, double scale) {
  const int64_t dim = table.size(1);
  const int64_t n = ids.numel();
  check_emb(table, ids, dim);
  debug_check_ids(ids, table.size(0));
  TORCH_CHECK(grad.is_cuda() && grad.is_contiguous() &&
              grad.numel() == n * dim, "grad shape mismatch");
  auto stream = c10::hip::getCurrentHIPStream().stream();
  float nls = (float)(-lr * scale);
  if (grad.scalar_type() == torch::kFloat32) {
    launch_row_segments(emb_bwd_sgd_kernel<F32Io, 16>,
                        emb_bwd_sgd_kernel<F32Io, 0>, n, dim, stream,
                        table.data_ptr<float>(), ids.data_ptr<int64_t>(),
                        grad.data_ptr<float>(), n, dim, nls);
  } else {
    TORCH_CHECK(grad.scalar_type() == torch::kBFloat16,
                "grad must be fp32 or bf16");
    launch_row_segments(emb_bwd_sgd_kernel<Bf16Io, 16>,
                        emb_bwd_sgd_kernel<Bf16Io, 0>, n, dim, stream,
                        table.data_ptr<float>(), ids.data_ptr<int64_t>(),
                        reinterpret_cast<unsigned short*>(grad.data_ptr()),
                        n, dim, nls);
  }
}

void emb_bwd_dense(torch::Tensor grad_table, torch::Tensor ids,
                   torch::Tensor grad, double scale) {
  const int64_t dim = grad_table.size(1);
  const int64_t n = ids.numel();
  check_emb(grad_table, ids, dim);
  debug_check_ids(ids, grad_table.size(0));
  TORCH_CHECK(grad.is_cuda() && grad.is_contiguous() &&
              grad.numel() == n * dim, "grad shape mismatch");
  auto stream = c10::hip::getCurrentHIPStream().stream();
  if (grad.scalar_type() == torch::kFloat32) {
    launch_row_segments(emb_bwd_dense_kernel<F32Io, 16>,
                        emb_bwd_dense_kernel<F32Io, 0>, n, dim, stream,
                        grad_table.data_ptr<float>(),
                        ids.data_ptr<int64_t>(), grad.data_ptr<float>(),
                        n, dim, (float)scale);
  } else {
    TORCH_CHECK(grad.scalar_type() == torch::kBFloat16,
                "grad must be fp32 or bf16");
    launch_row_segments(emb_bwd_dense_kernel<Bf16Io, 16>,
                        emb_bwd_dense_kernel<Bf16Io, 0>, n, dim, stream,
                        grad_table.data_ptr<float>(),
                        ids.data_ptr<int64_t>(),
                        reinterpret_cast<unsigned short*>(grad.data_ptr()),
                        n, dim, (float)scale);
  }
}

torch::Tensor emb_gather_sum(torch::Tensor table, torch::Tensor ids,
                             int64_t batch, bool out_bf16) {
  TORCH_CHECK(table.is_cuda() && table.is_contiguous() &&
              table.scalar_type() == torch::kFloat32,
              "table must be contiguous fp32 on GPU");
  TORCH_CHECK(ids.is_cuda() && ids.is_contiguous() &&
              ids.scalar_type() == torch::kInt64, "ids must be int64 GPU");
  TORCH_CHECK(ids.numel() % batch == 0, "ids size not divisible by batch");
  debug_check_ids(ids, table.numel());
  const int F = static_cast<int>(ids.numel() / batch);
  auto out = torch::empty({batch}, table.options().dtype(
      out_bf16 ? torch::kBFloat16 : torch::kFloat32));
  auto stream = c10::hip::getCurrentHIPStream().stream();
  int grid = miyarn_grid(batch);
  if (out_bf16) {
    hipLaunchKernelGGL(emb_gather_sum_kernel<Bf16Io>, dim3(grid),
                       dim3(MIYARN_BLOCK), 0, stream,
                       table.data_ptr<float>(), ids.data_ptr<int64_t>(),
                       reinterpret_cast<unsigned short*>(out.data_ptr()),
                       batch, F);
  } else {
    hipLaunchKernelGGL(emb_gather_sum_kernel<F32Io>, dim3(grid),
                       dim3(MIYARN_BLOCK), 0, stream,
                       table.data_ptr<float>(), ids.data_ptr<int64_t>(),
                       out.data_ptr<float>(), batch, F);
  }
  return out;
}

void emb_scatter_sum(torch::Tensor table, torch::Tensor ids,
                     torch::Tensor grad, double alpha) {
  TORCH_CHECK(table.is_cuda() && table.is_contiguous() &&
              table.scalar_type() == torch::kFloat32,
              "table must be contiguous fp32 on GPU");
  TORCH_CHECK(ids.is_cuda() && ids.is_contiguous() &&
              ids.scalar_type() == torch::kInt64, "ids must be int64 GPU");
  const int64_t batch = grad.numel();
  TORCH_CHECK(ids.numel() % batch == 0, "ids size not divisible by batch");
  debug_check_ids(ids, table.numel());
  const int F = static_cast<int>(ids.numel() / batch);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  int grid = miyarn_grid(batch * F);
  if (grad.scalar_type() == torch::kFloat32) {
    hipLaunchKernelGGL(emb_scatter_sum_kernel<F32Io>, dim3(grid),
                       dim3(MIYARN_BLOCK), 0, stream,
                       table.data_ptr<float>(), ids.data_ptr<int64_t>(),
                       grad.data_ptr<float>(), batch, F, (float)alpha);
  } else {
    TORCH_CHECK(grad.scalar_type() == torch::kBFloat16,
                "grad must be fp32 or bf16");
    hipLaunchKernelGGL(emb_scatter_sum_kernel<Bf16Io>, dim3(grid),
                       dim3(MIYARN_BLOCK), 0, stream,
                       table.data_ptr<float>(), ids.data_ptr<int64_t>(),
                       reinterpret_cast<unsigned short*>(grad.data_ptr()),
                       batch, F, (float)alpha);
  }
}

void emb_fwd_into(torch::Tensor table, torch::Tensor ids,
                  torch::Tensor out, int64_t col_offset) {
  const int64_t dim = table.size(1);
  const int64_t n = ids.numel();
  check_emb(table, ids, dim);
  debug_check_ids(ids, table.size(0));
  TORCH_CHECK(out.is_cuda() && out.is_contiguous() && out.dim() == 2,
              "out must be a contiguous 2D GPU tensor");
  TORCH_CHECK(dim % 4 == 0 && col_offset % 4 == 0 &&
              out.size(1) % 4 == 0,
              "emb_fwd_into needs dim, col_offset and out stride % 4 == 0");
  const int64_t batch = out.size(0);
  TORCH_CHECK(n % batch == 0, "ids not divisible by out rows");
  const int F = static_cast<int>(n / batch);
  TORCH_CHECK(col_offset + (int64_t)F * dim <= out.size(1),
              "slice out of range");
  auto stream = c10::hip::getCurrentHIPStream().stream();
  int grid = miyarn_grid(n * (dim / 4));
  if (out.scalar_type() == torch::kBFloat16) {
    hipLaunchKernelGGL(emb_fwd_into_kernel<Bf16Io>, dim3(grid),
                       dim3(MIYARN_BLOCK), 0, stream,
                       table.data_ptr<float>(), ids.data_ptr<int64_t>(),
                       reinterpret_cast<unsigned short*>(out.data_ptr()),
                       n, dim, F, out.size(1) / 4, col_offset / 4);
  } else {
    TORCH_CHECK(out.scalar_type() == torch::kFloat32, "fp32/bf16 only");
    hipLaunchKernelGGL(emb_fwd_into_kernel<F32Io>, dim3(grid),
                       dim3(MIYARN_BLOCK), 0, stream,
                       table.data_ptr<float>(), ids.data_ptr<int64_t>(),
                       out.data_ptr<float>(), n, dim, F,
                       out.size(1) / 4, col_offset / 4);
  }
}

// True when emb_lookup_fused_kernel covers the shape; the Python wrapper
// asks before it chooses between the kernel and the separate ops.
bool emb_lookup_fused_ok(int64_t dim, int64_t n_features, int64_t n_dense,
                         int64_t col_offset, int64_t out_cols) {
  return dim > 0 && dim % 4 == 0 && col_offset >= 0 &&
         col_offset % 4 == 0 && out_cols % 4 == 0 && n_dense >= 0 &&
         n_dense <= col_offset && n_features >= 1 &&
         n_features <= LOOKUP_LDS_FLOATS &&
         col_offset + n_features * dim <= out_cols &&
         // a chunk's quads are counted in an int
         LOOKUP_ROWS * (col_offset / 4 + n_features * (dim / 4)) <
             (int64_t(1) << 30);
}

// out[b, col_offset + f*dim + c] = table[ids[b, f] + offsets[f], c];
// out[b, :n_dense] = dense[b]; out[b, n_dense:col_offset] = 0; returns
// wide[b] = sum_f wide_table[ids[b, f] + offsets[f]] in out's dtype.
torch::Tensor emb_lookup_fused(torch::Tensor table, torch::Tensor wide_table,
                               torch::Tensor ids, torch::Tensor offsets,
                               c10::optional<torch::Tensor> dense,
                               torch::Tensor out, int64_t col_offset) {
  const int64_t dim = table.size(1);
  check_emb(table, ids, dim);
  TORCH_CHECK(ids.dim() == 2, "ids must be the raw [batch, features] array");
  const int64_t batch = ids.size(0);
  const int64_t F = ids.size(1);
  TORCH_CHECK(offsets.is_cuda() && offsets.is_contiguous() &&
              offsets.scalar_type() == torch::kInt64 &&
              offsets.numel() == F, "offsets must be int64 [features]");
  TORCH_CHECK(wide_table.is_cuda() && wide_table.is_contiguous() &&
              wide_table.scalar_type() == torch::kFloat32 &&
              wide_table.numel() == table.size(0), "bad wide table");
  TORCH_CHECK(out.is_cuda() && out.is_contiguous() && out.dim() == 2 &&
              out.size(0) == batch,
              "out must be a contiguous [batch, cols] GPU tensor");
  TORCH_CHECK(out.scalar_type() == torch::kBFloat16 ||
              out.scalar_type() == torch::kFloat32, "fp32/bf16 only");
  int64_t n_dense = 0;
  const void* dense_ptr = nullptr;
  if (dense.has_value()) {
    TORCH_CHECK(dense->is_cuda() && dense->is_contiguous() &&
                dense->dim() == 2 && dense->size(0) == batch &&
                dense->scalar_type() == out.scalar_type(),
                "dense must be contiguous [batch, n_dense] of out's dtype");
    n_dense = dense->size(1);
    dense_ptr = dense->data_ptr();
  }
  TORCH_CHECK(emb_lookup_fused_ok(dim, F, n_dense, col_offset, out.size(1)),
              "shape not covered by emb_lookup_fused (dim, col_offset and "
              "out stride % 4, n_dense <= col_offset, features <= ",
              LOOKUP_LDS_FLOATS, ")");
  if (bounds_debug_enabled())
    debug_check_ids(ids + offsets.unsqueeze(0), table.size(0));
  auto wide = torch::empty({batch}, out.options());
  if (batch == 0) return wide;
  const int rpc = static_cast<int>(
      std::min<int64_t>(LOOKUP_ROWS, LOOKUP_LDS_FLOATS / F));
  const int grid = static_cast<int>(std::min<int64_t>(
      (batch + rpc - 1) / rpc, MIYARN_MAX_BLOCKS));
  auto stream = c10::hip::getCurrentHIPStream().stream();
  auto launch = [&](auto io) {
    using Io = decltype(io);
    using S = typename Io::scalar_t;
    hipLaunchKernelGGL(emb_lookup_fused_kernel<Io>, dim3(grid),
                       dim3(MIYARN_BLOCK), 0, stream,
                       table.data_ptr<float>(), wide_table.data_ptr<float>(),
                       ids.data_ptr<int64_t>(), offsets.data_ptr<int64_t>(),
                       static_cast<const S*>(dense_ptr),
                       reinterpret_cast<S*>(out.data_ptr()),
                       reinterpret_cast<S*>(wide.data_ptr()), batch,
                       (int)dim, (int)F, rpc, out.size(1) / 4,
                       (int)(col_offset / 4), (int)n_dense);
  };
  if (out.scalar_type() == torch::kBFloat16)
    launch(Bf16Io{});
  else
    launch(F32Io{});
  return wide;
}

void emb_bwd_sgd_sorted(torch::Tensor table, torch::Tensor sorted_ids,
                        torch::Tensor grad, double lr, double scale) {
  const int64_t dim = table.size(1);
  const int64_t n = sorted_ids.numel();
  check_emb(table, sorted_ids, dim);
  debug_check_ids(sorted_ids, table.size(0));
  TORCH_CHECK(dim % 4 == 0, "sorted scatter needs dim % 4 == 0");
  TORCH_CHECK(grad.is_cuda() && grad.is_contiguous() &&
              grad.numel() == n * dim, "grad shape mismatch");
  auto stream = c10::hip::getCurrentHIPStream().stream();
  int grid = miyarn_grid_cap(n * (dim / 4), 8192);
  float nls = (float)(-lr * scale);
  if (grad.scalar_type() == torch::kFloat32) {
    hipLaunchKernelGGL(emb_bwd_sgd_sorted_kernel<F32Io>, dim3(grid),
                       dim3(MIYARN_BLOCK), 0, stream,
                       table.data_ptr<float>(),
                       sorted_ids.data_ptr<int64_t>(),
                       grad.data_ptr<float>(), n, dim, nls);
  } else {
    TORCH_CHECK(grad.scalar_type() == torch::kBFloat16,
                "grad must be fp32 or bf16");
    hipLaunchKernelGGL(emb_bwd_sgd_sorted_kernel<Bf16Io>, dim3(grid),
                       dim3(MIYARN_BLOCK), 0, stream,
                       table.data_ptr<float>(),
                       sorted_ids.data_ptr<int64_t>(),
                       reinterpret_cast<unsigned short*>(grad.data_ptr()),
                       n, dim, nls);
  }
}

// `grad` is a dense [n, dim] array, or a 2D view [gw.numel(), g_div * dim]
// whose rows are contiguous but lie a fixed stride apart (a column slice
// of a wider buffer): update row b * g_div + f then reads
// grad[b, f * dim : (f + 1) * dim] with no gather copy before the kernel.
// With `offsets` [g_div], `ids` holds the raw per-feature ids, row-major
// [gw.numel(), g_div], and update row b * g_div + f goes to table row
// ids[b, f] + offsets[f].
void emb_bwd_sgd_fused_wide_offs(torch::Tensor table,
                                 torch::Tensor wide_table, torch::Tensor ids,
                                 torch::Tensor grad, torch::Tensor gw,
                                 double lr, double scale,
                                 c10::optional<torch::Tensor> offsets) {
  const int64_t dim = table.size(1);
  const int64_t n = ids.numel();
  check_emb(table, ids, dim);
  if (offsets.has_value()) {
    TORCH_CHECK(offsets->is_cuda() && offsets->is_contiguous() &&
                offsets->scalar_type() == torch::kInt64 &&
                gw.numel() > 0 &&
                offsets->numel() * gw.numel() == n,
                "offsets must be int64 [ids.numel() / gw.numel()]");
    if (bounds_debug_enabled())
      debug_check_ids(ids.reshape({gw.numel(), offsets->numel()}) +
                          offsets->unsqueeze(0), table.size(0));
  } else {
    debug_check_ids(ids, table.size(0));
  }
  TORCH_CHECK(dim % 4 == 0, "fused wide update needs dim % 4 == 0");
  TORCH_CHECK(wide_table.is_cuda() && wide_table.is_contiguous() &&
              wide_table.scalar_type() == torch::kFloat32 &&
              wide_table.size(0) == table.size(0), "bad wide table");
  TORCH_CHECK(gw.is_cuda() && gw.is_contiguous() &&
              gw.scalar_type() == grad.scalar_type() &&
              gw.numel() > 0 && n % gw.numel() == 0,
              "gw dtype/shape mismatch");
  const int g_div = static_cast<int>(n / gw.numel());
  TORCH_CHECK(grad.is_cuda() && grad.numel() == n * dim,
              "grad shape mismatch");
  int64_t g_pad = 0;
  if (!grad.is_contiguous()) {
    TORCH_CHECK(grad.dim() == 2 && grad.size(0) == gw.numel() &&
                grad.size(1) == (int64_t)g_div * dim &&
                grad.stride(1) == 1 && grad.stride(0) >= grad.size(1),
                "a non-contiguous grad must be a row-strided "
                "[gw.numel(), g_div * dim] view");
    g_pad = grad.stride(0) - grad.size(1);
  }
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const float nls = (float)(-lr * scale);
  auto launch = [&](auto io) {
    using Io = decltype(io);
    using S = typename Io::scalar_t;
    auto* gp = reinterpret_cast<const S*>(grad.data_ptr());
    auto* gwp = reinterpret_cast<const S*>(gw.data_ptr());
    if (offsets.has_value()) {
      const int64_t* op = offsets->data_ptr<int64_t>();
      if (g_pad != 0)
        launch_row_segments(
            emb_bwd_sgd_fused_wide_offs_kernel<Io, 16, true>,
            emb_bwd_sgd_fused_wide_offs_kernel<Io, 0, true>, n, dim, stream,
            table.data_ptr<float>(), wide_table.data_ptr<float>(),
            ids.data_ptr<int64_t>(), op, gp, gwp, n, dim, g_div, g_pad, nls,
            nls);
      else
        launch_row_segments(
            emb_bwd_sgd_fused_wide_offs_kernel<Io, 16, false>,
            emb_bwd_sgd_fused_wide_offs_kernel<Io, 0, false>, n, dim, stream,
            table.data_ptr<float>(), wide_table.data_ptr<float>(),
            ids.data_ptr<int64_t>(), op, gp, gwp, n, dim, g_div, g_pad, nls,
            nls);
      return;
    }
    if (g_pad != 0)
      launch_row_segments(emb_bwd_sgd_fused_wide_kernel<Io, 16, true>,
                          emb_bwd_sgd_fused_wide_kernel<Io, 0, true>, n,
                          dim, stream, table.data_ptr<float>(),
                          wide_table.data_ptr<float>(),
                          ids.data_ptr<int64_t>(), gp, gwp, n, dim, g_div,
                          g_pad, nls, nls);
    else
      launch_row_segments(emb_bwd_sgd_fused_wide_kernel<Io, 16, false>,
                          emb_bwd_sgd_fused_wide_kernel<Io, 0, false>, n,
                          dim, stream, table.data_ptr<float>(),
                          wide_table.data_ptr<float>(),
                          ids.data_ptr<int64_t>(), gp, gwp, n, dim, g_div,
                          g_pad, nls, nls);
  };
  if (grad.scalar_type() == torch::kFloat32) {
    launch(F32Io{});
  } else {
    TORCH_CHECK(grad.scalar_type() == torch::kBFloat16, "fp32/bf16 only");
    launch(Bf16Io{});
  }
}

void emb_bwd_sgd_fused_wide(torch::Tensor table, torch::Tensor wide_table,
                            torch::Tensor ids, torch::Tensor grad,
                            torch::Tensor gw, double lr, double scale) {
  emb_bwd_sgd_fused_wide_offs(table, wide_table, ids, grad, gw, lr, scale,
                              c10::nullopt);
}
