// Sparse Adagrad for the embedding tables: accumulate, then claim.
//
// A stateful sparse optimizer must sum a batch's duplicate ids BEFORE it
// touches the state, then update state and weight once per unique row
// (torch.optim.Adagrad on a coalesced sparse gradient).  Pass 1 is the
// existing atomic scatter (emb_bwd_dense / emb_scatter_sum /
// emb_bwd_sgd_fused_wide with lr = -1) into a table-shaped fp32
// accumulator `acc` that is all-zero between calls.  Pass 2 (the kernels
// in this file) walks the SAME update list:
//
//  * one lane per update row does old = atomicExch(&stamp[id], epoch);
//    the row is won iff old != epoch (epoch is a host counter that
//    advances on every launch, so the stamp never needs clearing);
//  * the winner's lanes load the acc row, store zeros back (the
//    accumulator cleans itself), and read-modify-write state_sum and the
//    table with plain vector accesses; losers touch nothing.
//
// So every touched row is updated exactly once, with no float atomics and
// one returning exchange per update ROW (not per element).  The stamp is
// only ever accessed by device-scope atomics; acc/state/table are only
// read and written by the row's winner inside this launch, and the
// kernel boundary orders them against pass 1 and the next forward.
//
// Seam for other stateful sparse optimizers (Adam, FTRL, row-wise
// Adagrad): only `adagrad_one` knows the update rule.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include "common.h"

// pass 1 (embedding.hip)
void emb_bwd_dense(torch::Tensor grad_table, torch::Tensor ids,
                   torch::Tensor grad, double scale);
void emb_scatter_sum(torch::Tensor table, torch::Tensor ids,
                     torch::Tensor grad, double alpha);
void emb_bwd_sgd_fused_wide(torch::Tensor table, torch::Tensor wide_table,
                            torch::Tensor ids, torch::Tensor grad,
                            torch::Tensor gw, double lr, double scale);

namespace {

struct SparseAdagradArgs { float lr, eps; };

// g: summed, scaled gradient of one element; s, w: its state and weight
__device__ __forceinline__ void adagrad_one(float g, float* s, float* w,
                                            SparseAdagradArgs a) {
  *s += g * g;
  *w -= a.lr * g / (sqrtf(*s) + a.eps);
}

// Winner-side update of one 4-element quad: consume + zero the
// accumulator, then RMW state and weight.
__device__ __forceinline__ void adagrad_quad(float* __restrict__ acc,
                                             float* __restrict__ state,
                                             float* __restrict__ table,
                                             int64_t off,
                                             SparseAdagradArgs a) {
  float g[4], s[4], w[4];
  const float zero[4] = {0.f, 0.f, 0.f, 0.f};
  QuadIo<F32Io>::load4(acc, off >> 2, g);
  QuadIo<F32Io>::store4(acc, off >> 2, zero);
  QuadIo<F32Io>::load4(state, off >> 2, s);
  QuadIo<F32Io>::load4(table, off >> 2, w);
#pragma unroll
  for (int j = 0; j < 4; ++j) adagrad_one(g[j], &s[j], &w[j], a);
  QuadIo<F32Io>::store4(state, off >> 2, s);
  QuadIo<F32Io>::store4(table, off >> 2, w);
}

// (row, quad) map of emb_bwd_sgd_kernel, for dvec = dim/4 a power of two
// <= 64: a row's dvec lanes are then contiguous, aligned to dvec and
// inside one wave (block and grid stride are multiples of 64), so the
// c4 == 0 lane claims the row and a wave shuffle shares the verdict.
// The loop bound is block-uniform so every lane of a wave reaches the
// shuffle; lanes past `total` (tail wave) stay inactive and claim nothing.
// kWide: the row's winner also applies the dim-1 wide table that is
// driven by the same flat ids.
template <bool kWide>
__global__ void sparse_adagrad_apply_kernel(
    float* __restrict__ table, float* __restrict__ state,
    float* __restrict__ acc, float* __restrict__ wide_table,
    float* __restrict__ wide_state, float* __restrict__ wide_acc,
    int* __restrict__ stamp, const int64_t* __restrict__ ids,
    int64_t n_rows, int dshift, int epoch, SparseAdagradArgs a) {
  const int dvec = 1 << dshift;
  const int64_t dim = (int64_t)dvec << 2;
  const int64_t total = n_rows << dshift;
  const int64_t stride = gridDim.x * (int64_t)blockDim.x;
  const int lane = threadIdx.x & 63;
  const int c4 = threadIdx.x & (dvec - 1);
  for (int64_t base = blockIdx.x * (int64_t)blockDim.x; base < total;
       base += stride) {
    const int64_t t = base + threadIdx.x;
    const bool active = t < total;
    int64_t id = 0;
    int won = 0;
    if (active) {
      id = ids[t >> dshift];
      if (c4 == 0) won = atomicExch(&stamp[id], epoch) != epoch;
    }
    won = __shfl(won, lane - c4);
    if (!active || !won) continue;
    adagrad_quad(acc, state, table, id * dim + ((int64_t)c4 << 2), a);
    if (kWide && c4 == 0) {
      const float g = wide_acc[id];
      wide_acc[id] = 0.f;
      float s = wide_state[id], w = wide_table[id];
      adagrad_one(g, &s, &w, a);
      wide_state[id] = s;
      wide_table[id] = w;
    }
  }
}

// One lane per update row, any dim: the dim-1 wide table, and deep dims
// that fit neither dim % 4 == 0 nor the lane-sharing rule above (7, 12):
// correct, not fast for wide rows.
__global__ void sparse_adagrad_apply_row_kernel(
    float* __restrict__ table, float* __restrict__ state,
    float* __restrict__ acc, int* __restrict__ stamp,
    const int64_t* __restrict__ ids, int64_t n_rows, int64_t dim,
    int epoch, SparseAdagradArgs a) {
  const int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
       t < n_rows; t += stride) {
    const int64_t id = ids[t];
    if (atomicExch(&stamp[id], epoch) == epoch) continue;
    const int64_t off = id * dim;
    for (int64_t c = 0; c < dim; ++c) {
      const float g = acc[off + c];
      acc[off + c] = 0.f;
      float s = state[off + c], w = table[off + c];
      adagrad_one(g, &s, &w, a);
      state[off + c] = s;
      table[off + c] = w;
    }
  }
}

void check_f32_like(const torch::Tensor& t, const torch::Tensor& table,
                    const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
              t.scalar_type() == torch::kFloat32 &&
              t.numel() == table.numel(),
              name, " must be a contiguous fp32 GPU tensor shaped like "
              "its table");
}

void check_grad(const torch::Tensor& g, const char* name) {
  TORCH_CHECK(g.is_cuda() && g.is_contiguous() &&
              (g.scalar_type() == torch::kFloat32 ||
               g.scalar_type() == torch::kBFloat16),
              name, " must be a contiguous fp32 or bf16 GPU tensor");
}

// dim/4 as a shift when the quad kernel's lane-sharing rule holds, else -1
int quad_shift(int64_t dim) {
  if (dim % 4 != 0) return -1;
  const int64_t dvec = dim / 4;
  if (dvec > 64 || (dvec & (dvec - 1)) != 0) return -1;
  int s = 0;
  while ((int64_t(1) << s) < dvec) ++s;
  return s;
}

void check_apply(const torch::Tensor& table, const torch::Tensor& state_sum,
                 const torch::Tensor& acc, const torch::Tensor& stamp,
                 const torch::Tensor& ids, int64_t epoch) {
  TORCH_CHECK(table.is_cuda() && table.is_contiguous() &&
              table.dim() == 2 && table.scalar_type() == torch::kFloat32,
              "table must be a contiguous 2D fp32 GPU tensor");
  check_f32_like(state_sum, table, "state_sum");
  check_f32_like(acc, table, "acc");
  TORCH_CHECK(stamp.is_cuda() && stamp.is_contiguous() &&
              stamp.scalar_type() == torch::kInt32 &&
              stamp.numel() == table.size(0),
              "stamp must be contiguous int32 on GPU, one per table row");
  TORCH_CHECK(ids.is_cuda() && ids.is_contiguous() &&
              ids.scalar_type() == torch::kInt64,
              "ids must be contiguous int64 on GPU");
  TORCH_CHECK(epoch >= 1 && epoch < INT32_MAX,
              "epoch must be in [1, 2^31 - 1)");
}

void check_apply_fused_wide(
    const torch::Tensor& table, const torch::Tensor& state_sum,
    const torch::Tensor& acc, const torch::Tensor& wide_table,
    const torch::Tensor& wide_state, const torch::Tensor& wide_acc,
    const torch::Tensor& stamp, const torch::Tensor& ids, int64_t epoch) {
  check_apply(table, state_sum, acc, stamp, ids, epoch);
  TORCH_CHECK(wide_table.is_cuda() && wide_table.is_contiguous() &&
              wide_table.scalar_type() == torch::kFloat32 &&
              wide_table.numel() == table.size(0), "bad wide table");
  check_f32_like(wide_state, wide_table, "wide_state");
  check_f32_like(wide_acc, wide_table, "wide_acc");
  TORCH_CHECK(quad_shift(table.size(1)) >= 0,
              "fused wide Adagrad needs dim/4 to be a power of two <= 64");
}

void launch_apply(torch::Tensor& table, torch::Tensor& state_sum,
                  torch::Tensor& acc, torch::Tensor& stamp,
                  torch::Tensor& ids, int64_t epoch, double lr,
                  double eps) {
  const int64_t dim = table.size(1);
  const int64_t n = ids.numel();
  if (n == 0) return;
  SparseAdagradArgs a{(float)lr, (float)eps};
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const int shift = quad_shift(dim);
  if (shift >= 0) {
    int grid = miyarn_grid_cap(n << shift, 8192);
    hipLaunchKernelGGL(sparse_adagrad_apply_kernel<false>, dim3(grid),
                       dim3(MIYARN_BLOCK), 0, stream,
                       table.data_ptr<float>(), state_sum.data_ptr<float>(),
                       acc.data_ptr<float>(), (float*)nullptr,
                       (float*)nullptr, (float*)nullptr,
                       stamp.data_ptr<int>(), ids.data_ptr<int64_t>(), n,
                       shift, (int)epoch, a);
  } else {
    int grid = miyarn_grid_cap(n, 8192);
    hipLaunchKernelGGL(sparse_adagrad_apply_row_kernel, dim3(grid),
                       dim3(MIYARN_BLOCK), 0, stream,
                       table.data_ptr<float>(), state_sum.data_ptr<float>(),
                       acc.data_ptr<float>(), stamp.data_ptr<int>(),
                       ids.data_ptr<int64_t>(), n, dim, (int)epoch, a);
  }
}

void launch_apply_fused_wide(
    torch::Tensor& table, torch::Tensor& state_sum, torch::Tensor& acc,
    torch::Tensor& wide_table, torch::Tensor& wide_state,
    torch::Tensor& wide_acc, torch::Tensor& stamp, torch::Tensor& ids,
    int64_t epoch, double lr, double eps) {
  const int64_t n = ids.numel();
  if (n == 0) return;
  const int shift = quad_shift(table.size(1));
  SparseAdagradArgs a{(float)lr, (float)eps};
  auto stream = c10::hip::getCurrentHIPStream().stream();
  int grid = miyarn_grid_cap(n << shift, 8192);
  hipLaunchKernelGGL(sparse_adagrad_apply_kernel<true>, dim3(grid),
                     dim3(MIYARN_BLOCK), 0, stream,
                     table.data_ptr<float>(), state_sum.data_ptr<float>(),
                     acc.data_ptr<float>(), wide_table.data_ptr<float>(),
                     wide_state.data_ptr<float>(),
                     wide_acc.data_ptr<float>(), stamp.data_ptr<int>(),
                     ids.data_ptr<int64_t>(), n, shift, (int)epoch, a);
}

}  // namespace

// ---- pass 2 alone (acc already holds the summed, scaled gradient) ---------

void sparse_adagrad_apply(torch::Tensor table, torch::Tensor state_sum,
                          torch::Tensor acc, torch::Tensor stamp,
                          torch::Tensor ids, int64_t epoch, double lr,
                          double eps) {
  check_apply(table, state_sum, acc, stamp, ids, epoch);
  launch_apply(table, state_sum, acc, stamp, ids, epoch, lr, eps);
}

void sparse_adagrad_apply_fused_wide(
    torch::Tensor table, torch::Tensor state_sum, torch::Tensor acc,
    torch::Tensor wide_table, torch::Tensor wide_state,
    torch::Tensor wide_acc, torch::Tensor stamp, torch::Tensor ids,
    int64_t epoch, double lr, double eps) {
  check_apply_fused_wide(table, state_sum, acc, wide_table, wide_state,
                         wide_acc, stamp, ids, epoch);
  launch_apply_fused_wide(table, state_sum, acc, wide_table, wide_state,
                          wide_acc, stamp, ids, epoch, lr, eps);
}

// ---- pass 1 + pass 2: every input is validated before anything launches ---

// table[u] over the unique ids u: G = scale * sum of grad rows,
// state += G^2, table -= lr * G / (sqrt(state) + eps).
void emb_bwd_adagrad(torch::Tensor table, torch::Tensor state_sum,
                     torch::Tensor acc, torch::Tensor stamp,
                     torch::Tensor ids, torch::Tensor grad, int64_t epoch,
                     double lr, double eps, double scale) {
  check_apply(table, state_sum, acc, stamp, ids, epoch);
  check_grad(grad, "grad");
  TORCH_CHECK(grad.numel() == ids.numel() * table.size(1),
              "grad shape mismatch");
  emb_bwd_dense(acc, ids, grad, scale);
  launch_apply(table, state_sum, acc, stamp, ids, epoch, lr, eps);
}

// Wide companion: [rows, 1] table, per-example gradient gw with the
// gw[i / g_div] layout of emb_scatter_sum (g_div = ids.numel()/gw.numel()).
void emb_bwd_adagrad_wide(torch::Tensor table, torch::Tensor state_sum,
                          torch::Tensor acc, torch::Tensor stamp,
                          torch::Tensor ids, torch::Tensor gw,
                          int64_t epoch, double lr, double eps,
                          double scale) {
  check_apply(table, state_sum, acc, stamp, ids, epoch);
  TORCH_CHECK(table.size(1) == 1, "wide table must be [rows, 1]");
  check_grad(gw, "gw");
  TORCH_CHECK(gw.numel() > 0 ? ids.numel() % gw.numel() == 0
                             : ids.numel() == 0, "gw shape mismatch");
  if (ids.numel() == 0) return;
  emb_scatter_sum(acc, ids, gw, scale);
  launch_apply(table, state_sum, acc, stamp, ids, epoch, lr, eps);
}

// Deep + wide pair from one pass over the shared flat ids per phase.
void emb_bwd_adagrad_fused_wide(
    torch::Tensor table, torch::Tensor state_sum, torch::Tensor acc,
    torch::Tensor wide_table, torch::Tensor wide_state,
    torch::Tensor wide_acc, torch::Tensor stamp, torch::Tensor ids,
    torch::Tensor grad, torch::Tensor gw, int64_t epoch, double lr,
    double eps, double scale) {
  check_apply_fused_wide(table, state_sum, acc, wide_table, wide_state,
                         wide_acc, stamp, ids, epoch);
  check_grad(grad, "grad");
  check_grad(gw, "gw");
  TORCH_CHECK(grad.numel() == ids.numel() * table.size(1),
              "grad shape mismatch");
  TORCH_CHECK(gw.scalar_type() == grad.scalar_type() && gw.numel() > 0 &&
              ids.numel() % gw.numel() == 0, "gw dtype/shape mismatch");
  // lr = -1 turns the fused SGD scatter into acc += scale * g
  emb_bwd_sgd_fused_wide(acc, wide_acc, ids, grad, gw, -1.0, scale);
  launch_apply_fused_wide(table, state_sum, acc, wide_table, wide_state,
                          wide_acc, stamp, ids, epoch, lr, eps);
}
