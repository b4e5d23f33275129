// Stateful sparse optimizers for the embedding tables (Adagrad, FTRL,
// row-wise Adagrad): accumulate, then claim.
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
//    accumulator cleans itself), and read-modify-write the rule's state
//    and the table with plain vector accesses; losers touch nothing.
//
// So every touched row is updated exactly once, with no float atomics and
// one returning exchange per update ROW (not per element).  The stamp is
// only ever accessed by device-scope atomics; acc/state/table are only
// read and written by the row's winner inside this launch, and the
// kernel boundary orders them against pass 1 and the next forward.
//
// The update rule is a template parameter of pass 2.  A rule type has
//   struct Args            its scalars, passed by value;
//   kStates                how many table-shaped fp32 state tensors;
//   one(g, s, w, a)        the per-element update: g the summed, scaled
//                          gradient, s[kStates] the states, w the weight.
// AdagradRule (1 state) and FtrlRule (2 states) are instantiated.  That
// interface is per ELEMENT with table-shaped states: lazy Adam would be one
// more such struct plus entry points; row-wise Adagrad is not.
//
// Row-wise Adagrad keeps ONE fp32 accumulator per row, state_row[rows]:
//   m = (sum_c G[u, c]^2) / dim;  state_row[u] += m;
//   table[u, :] -= lr * G[u, :] / (sqrt(state_row[u]) + eps).
// It needs a reduction over the row before any element can move, and its
// state is not shaped like its table, so it has pass-2 kernels of its own
// (rowwise_adagrad_apply_kernel / _row_kernel below) on the same claim and
// the same (row, quad) map, next to the element-wise template and sharing
// only rule_elem (the wide companion) with it.  In the lane-sharing
// kernel the row's dvec lanes complete the sum of squares with a
// __shfl_xor butterfly (steps 1 .. dvec/2).  Every one of the row's lanes
// then reads the old state_row[id] itself, rather than one lane reading it
// and a shuffle broadcasting it: the lanes of a row share one address, so
// the wave's load instruction asks for one 4-byte word per row either way,
// it is issued together with the accumulator loads instead of behind
// them, and a broadcast would put one more cross-lane operation and one
// more wait on the path from the loads to the table store.  The butterfly
// is symmetric (a + b == b + a at every step), so all lanes of a row hold
// the same bits of the sum and of the new state; the quad-0 lane stores it.
// The one-lane-per-row kernel makes two trips over the row: the first sums
// the squares, the second re-reads the accumulator (the lane's own lines,
// just fetched), zeroes it and applies the update; zeroing in the first
// trip would lose G.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <vector>
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

struct AdagradRule {
  struct Args { float lr, eps; };
  static constexpr int kStates = 1;  // state_sum
  __device__ static __forceinline__ void one(float g, float (&s)[1],
                                             float* w, Args a) {
    s[0] += g * g;
    *w -= a.lr * g / (sqrtf(s[0]) + a.eps);
  }
};

// FTRL-proximal, learning_rate_power = -0.5, no beta, no L2 shrinkage
// (TF Ftrl); s[0] = n (accum), s[1] = z (linear).
//
// No clamp on the division: q == 0 needs n' == 0 and l2 == 0.  Then
// g == 0 and n == 0, so z' == z, and z is 0 for any state this rule
// itself produced (z only ever moves together with n).  |z'| > l1 is then
// false for every l1 >= 0 and the exact-zero branch is taken, so no
// division by zero happens.  lr > 0, l1 >= 0, l2 >= 0 are host-checked.
struct FtrlRule {
  struct Args { float lr, l1, l2; };
  static constexpr int kStates = 2;  // accum, linear
  __device__ static __forceinline__ void one(float g, float (&s)[2],
                                             float* w, Args a) {
    const float n_new = s[0] + g * g;
    const float r_new = sqrtf(n_new);
    const float z = s[1] + g - (r_new - sqrtf(s[0])) / a.lr * *w;
    const float q = r_new / a.lr + 2.f * a.l2;
    s[0] = n_new;
    s[1] = z;
    *w = fabsf(z) > a.l1 ? (copysignf(a.l1, z) - z) / q : 0.f;
  }
};

// Stand-in for "no wide companion" in the pair kernel.
struct NoRule {
  struct Args {};
  static constexpr int kStates = 0;
};

// The state tensors of one table, as a kernel argument.
template <int N> struct StatePtrs { float* p[N > 0 ? N : 1]; };

// Winner-side update of one 4-element quad: consume + zero the
// accumulator, then RMW the states and the weight.
template <typename Rule>
__device__ __forceinline__ void rule_quad(
    float* __restrict__ acc, const StatePtrs<Rule::kStates>& st,
    float* __restrict__ table, int64_t off, typename Rule::Args a) {
  constexpr int K = Rule::kStates;
  float g[4], w[4], s[K][4];
  const float zero[4] = {0.f, 0.f, 0.f, 0.f};
  QuadIo<F32Io>::load4(acc, off >> 2, g);
  QuadIo<F32Io>::store4(acc, off >> 2, zero);
#pragma unroll
  for (int k = 0; k < K; ++k) QuadIo<F32Io>::load4(st.p[k], off >> 2, s[k]);
  QuadIo<F32Io>::load4(table, off >> 2, w);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float e[K];
#pragma unroll
    for (int k = 0; k < K; ++k) e[k] = s[k][j];
    Rule::one(g[j], e, &w[j], a);
#pragma unroll
    for (int k = 0; k < K; ++k) s[k][j] = e[k];
  }
#pragma unroll
  for (int k = 0; k < K; ++k) QuadIo<F32Io>::store4(st.p[k], off >> 2, s[k]);
  QuadIo<F32Io>::store4(table, off >> 2, w);
}

// The same for one element (wide scalar, one-lane-per-row kernel).
template <typename Rule>
__device__ __forceinline__ void rule_elem(
    float* __restrict__ acc, const StatePtrs<Rule::kStates>& st,
    float* __restrict__ table, int64_t i, typename Rule::Args a) {
  constexpr int K = Rule::kStates;
  const float g = acc[i];
  acc[i] = 0.f;
  float e[K], w = table[i];
#pragma unroll
  for (int k = 0; k < K; ++k) e[k] = st.p[k][i];
  Rule::one(g, e, &w, a);
#pragma unroll
  for (int k = 0; k < K; ++k) st.p[k][i] = e[k];
  table[i] = w;
}

// (row, quad) map of emb_bwd_sgd_kernel, for dvec = dim/4 a power of two
// <= 64: a row's dvec lanes are then contiguous, aligned to dvec and
// inside one wave (block and grid stride are multiples of 64), so the
// c4 == 0 lane claims the row and a wave shuffle shares the verdict.
// The loop bound is block-uniform so every lane of a wave reaches the
// shuffle; lanes past `total` (tail wave) stay inactive and claim nothing.
// WideRule != NoRule: the row's winner also applies the dim-1 wide table
// that is driven by the same flat ids, under its own rule and args.
template <typename Rule, typename WideRule>
__global__ void sparse_adagrad_apply_kernel(
    float* __restrict__ table, StatePtrs<Rule::kStates> state,
    float* __restrict__ acc, float* __restrict__ wide_table,
    StatePtrs<WideRule::kStates> wide_state, float* __restrict__ wide_acc,
    int* __restrict__ stamp, const int64_t* __restrict__ ids,
    int64_t n_rows, int dshift, int epoch, typename Rule::Args a,
    typename WideRule::Args wa) {
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
    rule_quad<Rule>(acc, state, table, id * dim + ((int64_t)c4 << 2), a);
    if constexpr (WideRule::kStates > 0) {
      if (c4 == 0)
        rule_elem<WideRule>(wide_acc, wide_state, wide_table, id, wa);
    }
  }
}

// One lane per update row, any dim: the dim-1 wide table, and deep dims
// that fit neither dim % 4 == 0 nor the lane-sharing rule above (7, 12):
// correct, not fast for wide rows.
template <typename Rule>
__global__ void sparse_adagrad_apply_row_kernel(
    float* __restrict__ table, StatePtrs<Rule::kStates> state,
    float* __restrict__ acc, int* __restrict__ stamp,
    const int64_t* __restrict__ ids, int64_t n_rows, int64_t dim,
    int epoch, typename Rule::Args a) {
  const int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
       t < n_rows; t += stride) {
    const int64_t id = ids[t];
    if (atomicExch(&stamp[id], epoch) == epoch) continue;
    const int64_t off = id * dim;
    for (int64_t c = 0; c < dim; ++c)
      rule_elem<Rule>(acc, state, table, off + c, a);
  }
}

// ---- row-wise Adagrad -------------------------------------------------------

// The (row, quad) map and claim of sparse_adagrad_apply_kernel.  Unlike
// there, nobody leaves the iteration before the butterfly: every shuffle
// is reached by all 64 lanes of the wave (losers and the inactive lanes of
// a tail wave contribute zeros to their own rows' sums, which nobody uses),
// so the loads sit inside `mine` and the shuffles outside it.  A row's
// dvec lanes are contiguous and aligned to dvec, so lane ^ m for m < dvec
// stays inside the row.
template <typename WideRule>
__global__ void rowwise_adagrad_apply_kernel(
    float* __restrict__ table, float* __restrict__ state_row,
    float* __restrict__ acc, float* __restrict__ wide_table,
    StatePtrs<WideRule::kStates> wide_state, float* __restrict__ wide_acc,
    int* __restrict__ stamp, const int64_t* __restrict__ ids,
    int64_t n_rows, int dshift, int epoch, AdagradRule::Args a,
    typename WideRule::Args wa) {
  const int dvec = 1 << dshift;
  const int64_t dim = (int64_t)dvec << 2;
  const int64_t total = n_rows << dshift;
  const int64_t stride = gridDim.x * (int64_t)blockDim.x;
  const int lane = threadIdx.x & 63;
  const int c4 = threadIdx.x & (dvec - 1);
  const float zero[4] = {0.f, 0.f, 0.f, 0.f};
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
    const bool mine = active && won;
    const int64_t q = (id * dim >> 2) + c4;
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    float s = 0.f;
    if (mine) {
      QuadIo<F32Io>::load4(acc, q, g);
      QuadIo<F32Io>::store4(acc, q, zero);
      s = state_row[id];
    }
    float ss = g[0] * g[0] + g[1] * g[1] + g[2] * g[2] + g[3] * g[3];
    for (int m = 1; m < dvec; m <<= 1) ss += __shfl_xor(ss, m);
    if (!mine) continue;
    s += ss / (float)dim;
    const float denom = sqrtf(s) + a.eps;
    float w[4];
    QuadIo<F32Io>::load4(table, q, w);
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] -= a.lr * g[j] / denom;
    QuadIo<F32Io>::store4(table, q, w);
    if (c4 == 0) {
      state_row[id] = s;
      if constexpr (WideRule::kStates > 0)
        rule_elem<WideRule>(wide_acc, wide_state, wide_table, id, wa);
    }
  }
}

// One lane per update row, any dim (1, 7, 12, 512): two trips over the row.
__global__ void rowwise_adagrad_apply_row_kernel(
    float* __restrict__ table, float* __restrict__ state_row,
    float* __restrict__ acc, int* __restrict__ stamp,
    const int64_t* __restrict__ ids, int64_t n_rows, int64_t dim,
    int epoch, AdagradRule::Args a) {
  const int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
       t < n_rows; t += stride) {
    const int64_t id = ids[t];
    if (atomicExch(&stamp[id], epoch) == epoch) continue;
    const int64_t off = id * dim;
    float ss = 0.f;
    for (int64_t c = 0; c < dim; ++c) ss += acc[off + c] * acc[off + c];
    const float s = state_row[id] + ss / (float)dim;
    state_row[id] = s;
    const float denom = sqrtf(s) + a.eps;
    for (int64_t c = 0; c < dim; ++c) {
      const float g = acc[off + c];
      acc[off + c] = 0.f;
      table[off + c] -= a.lr * g / denom;
    }
  }
}

// ---- host: checks -----------------------------------------------------------

using Tensors = std::vector<torch::Tensor>;

void check_f32_like(const torch::Tensor& t, const torch::Tensor& table,
                    const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
              t.scalar_type() == torch::kFloat32 &&
              t.numel() == table.numel(),
              name, " must be a contiguous fp32 GPU tensor shaped like "
              "its table");
}

// row-wise Adagrad's state: one value per table row, not per element
void check_row_state(const torch::Tensor& t, const torch::Tensor& table) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
              t.scalar_type() == torch::kFloat32 &&
              t.numel() == table.size(0),
              "state_row must be a contiguous fp32 GPU tensor with one "
              "value per table row");
}

void check_grad(const torch::Tensor& g, const char* name) {
  TORCH_CHECK(g.is_cuda() && g.is_contiguous() &&
              (g.scalar_type() == torch::kFloat32 ||
               g.scalar_type() == torch::kBFloat16),
              name, " must be a contiguous fp32 or bf16 GPU tensor");
}

void check_ftrl_args(double lr, double l1, double l2) {
  TORCH_CHECK(lr > 0.0, "FTRL needs lr > 0");
  TORCH_CHECK(l1 >= 0.0 && l2 >= 0.0, "FTRL needs l1 >= 0 and l2 >= 0");
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

// `states`: the rule's state tensors, in the rule's order
void check_apply(const torch::Tensor& table, const Tensors& states,
                 const torch::Tensor& acc, const torch::Tensor& stamp,
                 const torch::Tensor& ids, int64_t epoch) {
  TORCH_CHECK(table.is_cuda() && table.is_contiguous() &&
              table.dim() == 2 && table.scalar_type() == torch::kFloat32,
              "table must be a contiguous 2D fp32 GPU tensor");
  for (const auto& s : states) check_f32_like(s, table, "state");
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
    const torch::Tensor& table, const Tensors& states,
    const torch::Tensor& acc, const torch::Tensor& wide_table,
    const Tensors& wide_states, const torch::Tensor& wide_acc,
    const torch::Tensor& stamp, const torch::Tensor& ids, int64_t epoch) {
  check_apply(table, states, acc, stamp, ids, epoch);
  TORCH_CHECK(wide_table.is_cuda() && wide_table.is_contiguous() &&
              wide_table.scalar_type() == torch::kFloat32 &&
              wide_table.numel() == table.size(0), "bad wide table");
  for (const auto& s : wide_states)
    check_f32_like(s, wide_table, "wide state");
  check_f32_like(wide_acc, wide_table, "wide_acc");
  TORCH_CHECK(quad_shift(table.size(1)) >= 0,
              "the fused deep+wide apply needs dim/4 to be a power of two "
              "<= 64");
}

void check_deep_grad(const torch::Tensor& table, const torch::Tensor& ids,
                     const torch::Tensor& grad) {
  check_grad(grad, "grad");
  TORCH_CHECK(grad.numel() == ids.numel() * table.size(1),
              "grad shape mismatch");
}

void check_wide_grad(const torch::Tensor& table, const torch::Tensor& ids,
                     const torch::Tensor& gw) {
  TORCH_CHECK(table.size(1) == 1, "wide table must be [rows, 1]");
  check_grad(gw, "gw");
  TORCH_CHECK(gw.numel() > 0 ? ids.numel() % gw.numel() == 0
                             : ids.numel() == 0, "gw shape mismatch");
}

void check_pair_grads(const torch::Tensor& table, const torch::Tensor& ids,
                      const torch::Tensor& grad, const torch::Tensor& gw) {
  check_deep_grad(table, ids, grad);
  check_grad(gw, "gw");
  TORCH_CHECK(gw.scalar_type() == grad.scalar_type() && gw.numel() > 0 &&
              ids.numel() % gw.numel() == 0, "gw dtype/shape mismatch");
}

// ---- host: launches (inputs already checked) --------------------------------

template <int N> StatePtrs<N> state_ptrs(const Tensors& states) {
  StatePtrs<N> p{};
  for (int k = 0; k < N; ++k) p.p[k] = states[k].data_ptr<float>();
  return p;
}

template <typename Rule>
void launch_apply(torch::Tensor& table, const Tensors& states,
                  torch::Tensor& acc, torch::Tensor& stamp,
                  torch::Tensor& ids, int64_t epoch,
                  typename Rule::Args a) {
  const int64_t dim = table.size(1);
  const int64_t n = ids.numel();
  if (n == 0) return;
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const auto st = state_ptrs<Rule::kStates>(states);
  const int shift = quad_shift(dim);
  if (shift >= 0) {
    int grid = miyarn_grid_cap(n << shift, 8192);
    hipLaunchKernelGGL((sparse_adagrad_apply_kernel<Rule, NoRule>),
                       dim3(grid), dim3(MIYARN_BLOCK), 0, stream,
                       table.data_ptr<float>(), st, acc.data_ptr<float>(),
                       (float*)nullptr, StatePtrs<0>{}, (float*)nullptr,
                       stamp.data_ptr<int>(), ids.data_ptr<int64_t>(), n,
                       shift, (int)epoch, a, NoRule::Args{});
  } else {
    int grid = miyarn_grid_cap(n, 8192);
    hipLaunchKernelGGL(sparse_adagrad_apply_row_kernel<Rule>, dim3(grid),
                       dim3(MIYARN_BLOCK), 0, stream,
                       table.data_ptr<float>(), st, acc.data_ptr<float>(),
                       stamp.data_ptr<int>(), ids.data_ptr<int64_t>(), n,
                       dim, (int)epoch, a);
  }
}

template <typename Rule, typename WideRule>
void launch_apply_fused_wide(
    torch::Tensor& table, const Tensors& states, torch::Tensor& acc,
    torch::Tensor& wide_table, const Tensors& wide_states,
    torch::Tensor& wide_acc, torch::Tensor& stamp, torch::Tensor& ids,
    int64_t epoch, typename Rule::Args a, typename WideRule::Args wa) {
  const int64_t n = ids.numel();
  if (n == 0) return;
  const int shift = quad_shift(table.size(1));
  auto stream = c10::hip::getCurrentHIPStream().stream();
  int grid = miyarn_grid_cap(n << shift, 8192);
  hipLaunchKernelGGL((sparse_adagrad_apply_kernel<Rule, WideRule>),
                     dim3(grid), dim3(MIYARN_BLOCK), 0, stream,
                     table.data_ptr<float>(),
                     state_ptrs<Rule::kStates>(states),
                     acc.data_ptr<float>(), wide_table.data_ptr<float>(),
                     state_ptrs<WideRule::kStates>(wide_states),
                     wide_acc.data_ptr<float>(), stamp.data_ptr<int>(),
                     ids.data_ptr<int64_t>(), n, shift, (int)epoch, a, wa);
}

AdagradRule::Args adagrad_args(double lr, double eps) {
  return {(float)lr, (float)eps};
}

FtrlRule::Args ftrl_args(double lr, double l1, double l2) {
  return {(float)lr, (float)l1, (float)l2};
}

// ---- row-wise Adagrad: checks and launches ----------------------------------

void check_rowwise_apply(const torch::Tensor& table,
                         const torch::Tensor& state_row,
                         const torch::Tensor& acc,
                         const torch::Tensor& stamp,
                         const torch::Tensor& ids, int64_t epoch) {
  check_apply(table, {}, acc, stamp, ids, epoch);
  check_row_state(state_row, table);
}

void check_rowwise_apply_fused_wide(
    const torch::Tensor& table, const torch::Tensor& state_row,
    const torch::Tensor& acc, const torch::Tensor& wide_table,
    const Tensors& wide_states, const torch::Tensor& wide_acc,
    const torch::Tensor& stamp, const torch::Tensor& ids, int64_t epoch) {
  check_apply_fused_wide(table, {}, acc, wide_table, wide_states, wide_acc,
                         stamp, ids, epoch);
  check_row_state(state_row, table);
}

void launch_rowwise_apply(torch::Tensor& table, torch::Tensor& state_row,
                          torch::Tensor& acc, torch::Tensor& stamp,
                          torch::Tensor& ids, int64_t epoch,
                          AdagradRule::Args a) {
  const int64_t dim = table.size(1);
  const int64_t n = ids.numel();
  if (n == 0) return;
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const int shift = quad_shift(dim);
  if (shift >= 0) {
    int grid = miyarn_grid_cap(n << shift, 8192);
    hipLaunchKernelGGL(rowwise_adagrad_apply_kernel<NoRule>, dim3(grid),
                       dim3(MIYARN_BLOCK), 0, stream,
                       table.data_ptr<float>(), state_row.data_ptr<float>(),
                       acc.data_ptr<float>(), (float*)nullptr,
                       StatePtrs<0>{}, (float*)nullptr,
                       stamp.data_ptr<int>(), ids.data_ptr<int64_t>(), n,
                       shift, (int)epoch, a, NoRule::Args{});
  } else {
    int grid = miyarn_grid_cap(n, 8192);
    hipLaunchKernelGGL(rowwise_adagrad_apply_row_kernel, dim3(grid),
                       dim3(MIYARN_BLOCK), 0, stream,
                       table.data_ptr<float>(), state_row.data_ptr<float>(),
                       acc.data_ptr<float>(), stamp.data_ptr<int>(),
                       ids.data_ptr<int64_t>(), n, dim, (int)epoch, a);
  }
}

template <typename WideRule>
void launch_rowwise_apply_fused_wide(
    torch::Tensor& table, torch::Tensor& state_row, torch::Tensor& acc,
    torch::Tensor& wide_table, const Tensors& wide_states,
    torch::Tensor& wide_acc, torch::Tensor& stamp, torch::Tensor& ids,
    int64_t epoch, AdagradRule::Args a, typename WideRule::Args wa) {
  const int64_t n = ids.numel();
  if (n == 0) return;
  const int shift = quad_shift(table.size(1));
  auto stream = c10::hip::getCurrentHIPStream().stream();
  int grid = miyarn_grid_cap(n << shift, 8192);
  hipLaunchKernelGGL(rowwise_adagrad_apply_kernel<WideRule>, dim3(grid),
                     dim3(MIYARN_BLOCK), 0, stream,
                     table.data_ptr<float>(), state_row.data_ptr<float>(),
                     acc.data_ptr<float>(), wide_table.data_ptr<float>(),
                     state_ptrs<WideRule::kStates>(wide_states),
                     wide_acc.data_ptr<float>(), stamp.data_ptr<int>(),
                     ids.data_ptr<int64_t>(), n, shift, (int)epoch, a, wa);
}

}  // namespace

// ---- pass 2 alone (acc already holds the summed, scaled gradient) ---------

void sparse_adagrad_apply(torch::Tensor table, torch::Tensor state_sum,
                          torch::Tensor acc, torch::Tensor stamp,
                          torch::Tensor ids, int64_t epoch, double lr,
                          double eps) {
  check_apply(table, {state_sum}, acc, stamp, ids, epoch);
  launch_apply<AdagradRule>(table, {state_sum}, acc, stamp, ids, epoch,
                            adagrad_args(lr, eps));
}

void sparse_adagrad_apply_fused_wide(
    torch::Tensor table, torch::Tensor state_sum, torch::Tensor acc,
    torch::Tensor wide_table, torch::Tensor wide_state,
    torch::Tensor wide_acc, torch::Tensor stamp, torch::Tensor ids,
    int64_t epoch, double lr, double eps) {
  check_apply_fused_wide(table, {state_sum}, acc, wide_table, {wide_state},
                         wide_acc, stamp, ids, epoch);
  launch_apply_fused_wide<AdagradRule, AdagradRule>(
      table, {state_sum}, acc, wide_table, {wide_state}, wide_acc, stamp,
      ids, epoch, adagrad_args(lr, eps), adagrad_args(lr, eps));
}

void sparse_ftrl_apply(torch::Tensor table, torch::Tensor accum,
                       torch::Tensor linear, torch::Tensor acc,
                       torch::Tensor stamp, torch::Tensor ids,
                       int64_t epoch, double lr, double l1, double l2) {
  check_ftrl_args(lr, l1, l2);
  check_apply(table, {accum, linear}, acc, stamp, ids, epoch);
  launch_apply<FtrlRule>(table, {accum, linear}, acc, stamp, ids, epoch,
                         ftrl_args(lr, l1, l2));
}

// deep Adagrad (lr, eps) + wide FTRL (wide_lr, l1, l2)
void sparse_adagrad_ftrl_apply_fused_wide(
    torch::Tensor table, torch::Tensor state_sum, torch::Tensor acc,
    torch::Tensor wide_table, torch::Tensor wide_accum,
    torch::Tensor wide_linear, torch::Tensor wide_acc, torch::Tensor stamp,
    torch::Tensor ids, int64_t epoch, double lr, double eps,
    double wide_lr, double l1, double l2) {
  check_ftrl_args(wide_lr, l1, l2);
  check_apply_fused_wide(table, {state_sum}, acc, wide_table,
                         {wide_accum, wide_linear}, wide_acc, stamp, ids,
                         epoch);
  launch_apply_fused_wide<AdagradRule, FtrlRule>(
      table, {state_sum}, acc, wide_table, {wide_accum, wide_linear},
      wide_acc, stamp, ids, epoch, adagrad_args(lr, eps),
      ftrl_args(wide_lr, l1, l2));
}

// deep FTRL (lr, l1, l2) + wide FTRL (wide_lr, l1, l2)
void sparse_ftrl_apply_fused_wide(
    torch::Tensor table, torch::Tensor accum, torch::Tensor linear,
    torch::Tensor acc, torch::Tensor wide_table, torch::Tensor wide_accum,
    torch::Tensor wide_linear, torch::Tensor wide_acc, torch::Tensor stamp,
    torch::Tensor ids, int64_t epoch, double lr, double wide_lr, double l1,
    double l2) {
  check_ftrl_args(lr, l1, l2);
  check_ftrl_args(wide_lr, l1, l2);
  check_apply_fused_wide(table, {accum, linear}, acc, wide_table,
                         {wide_accum, wide_linear}, wide_acc, stamp, ids,
                         epoch);
  launch_apply_fused_wide<FtrlRule, FtrlRule>(
      table, {accum, linear}, acc, wide_table, {wide_accum, wide_linear},
      wide_acc, stamp, ids, epoch, ftrl_args(lr, l1, l2),
      ftrl_args(wide_lr, l1, l2));
}

// row-wise Adagrad, single table
void sparse_rowwise_adagrad_apply(torch::Tensor table,
                                  torch::Tensor state_row,
                                  torch::Tensor acc, torch::Tensor stamp,
                                  torch::Tensor ids, int64_t epoch,
                                  double lr, double eps) {
  check_rowwise_apply(table, state_row, acc, stamp, ids, epoch);
  launch_rowwise_apply(table, state_row, acc, stamp, ids, epoch,
                       adagrad_args(lr, eps));
}

// deep row-wise Adagrad + wide Adagrad, one (lr, eps)
void sparse_rowwise_adagrad_apply_fused_wide(
    torch::Tensor table, torch::Tensor state_row, torch::Tensor acc,
    torch::Tensor wide_table, torch::Tensor wide_state,
    torch::Tensor wide_acc, torch::Tensor stamp, torch::Tensor ids,
    int64_t epoch, double lr, double eps) {
  check_rowwise_apply_fused_wide(table, state_row, acc, wide_table,
                                 {wide_state}, wide_acc, stamp, ids, epoch);
  launch_rowwise_apply_fused_wide<AdagradRule>(
      table, state_row, acc, wide_table, {wide_state}, wide_acc, stamp, ids,
      epoch, adagrad_args(lr, eps), adagrad_args(lr, eps));
}

// deep row-wise Adagrad (lr, eps) + wide FTRL (wide_lr, l1, l2)
void sparse_rowwise_adagrad_ftrl_apply_fused_wide(
    torch::Tensor table, torch::Tensor state_row, torch::Tensor acc,
    torch::Tensor wide_table, torch::Tensor wide_accum,
    torch::Tensor wide_linear, torch::Tensor wide_acc, torch::Tensor stamp,
    torch::Tensor ids, int64_t epoch, double lr, double eps,
    double wide_lr, double l1, double l2) {
  check_ftrl_args(wide_lr, l1, l2);
  check_rowwise_apply_fused_wide(table, state_row, acc, wide_table,
                                 {wide_accum, wide_linear}, wide_acc, stamp,
                                 ids, epoch);
  launch_rowwise_apply_fused_wide<FtrlRule>(
      table, state_row, acc, wide_table, {wide_accum, wide_linear},
      wide_acc, stamp, ids, epoch, adagrad_args(lr, eps),
      ftrl_args(wide_lr, l1, l2));
}

// ---- pass 1 + pass 2: every input is validated before anything launches ---

// table[u] over the unique ids u: G = scale * sum of grad rows,
// state += G^2, table -= lr * G / (sqrt(state) + eps).
void emb_bwd_adagrad(torch::Tensor table, torch::Tensor state_sum,
                     torch::Tensor acc, torch::Tensor stamp,
                     torch::Tensor ids, torch::Tensor grad, int64_t epoch,
                     double lr, double eps, double scale) {
  check_apply(table, {state_sum}, acc, stamp, ids, epoch);
  check_deep_grad(table, ids, grad);
  emb_bwd_dense(acc, ids, grad, scale);
  launch_apply<AdagradRule>(table, {state_sum}, acc, stamp, ids, epoch,
                            adagrad_args(lr, eps));
}

// Wide companion: [rows, 1] table, per-example gradient gw with the
// gw[i / g_div] layout of emb_scatter_sum (g_div = ids.numel()/gw.numel()).
void emb_bwd_adagrad_wide(torch::Tensor table, torch::Tensor state_sum,
                          torch::Tensor acc, torch::Tensor stamp,
                          torch::Tensor ids, torch::Tensor gw,
                          int64_t epoch, double lr, double eps,
                          double scale) {
  check_apply(table, {state_sum}, acc, stamp, ids, epoch);
  check_wide_grad(table, ids, gw);
  if (ids.numel() == 0) return;
  emb_scatter_sum(acc, ids, gw, scale);
  launch_apply<AdagradRule>(table, {state_sum}, acc, stamp, ids, epoch,
                            adagrad_args(lr, eps));
}

// Deep + wide pair from one pass over the shared flat ids per phase.
void emb_bwd_adagrad_fused_wide(
    torch::Tensor table, torch::Tensor state_sum, torch::Tensor acc,
    torch::Tensor wide_table, torch::Tensor wide_state,
    torch::Tensor wide_acc, torch::Tensor stamp, torch::Tensor ids,
    torch::Tensor grad, torch::Tensor gw, int64_t epoch, double lr,
    double eps, double scale) {
  check_apply_fused_wide(table, {state_sum}, acc, wide_table, {wide_state},
                         wide_acc, stamp, ids, epoch);
  check_pair_grads(table, ids, grad, gw);
  // lr = -1 turns the fused SGD scatter into acc += scale * g
  emb_bwd_sgd_fused_wide(acc, wide_acc, ids, grad, gw, -1.0, scale);
  launch_apply_fused_wide<AdagradRule, AdagradRule>(
      table, {state_sum}, acc, wide_table, {wide_state}, wide_acc, stamp,
      ids, epoch, adagrad_args(lr, eps), adagrad_args(lr, eps));
}

// FTRL-proximal on the unique ids u: G as above, then FtrlRule::one per
// element on (accum, linear, table).
void emb_bwd_ftrl(torch::Tensor table, torch::Tensor accum,
                  torch::Tensor linear, torch::Tensor acc,
                  torch::Tensor stamp, torch::Tensor ids,
                  torch::Tensor grad, int64_t epoch, double lr, double l1,
                  double l2, double scale) {
  check_ftrl_args(lr, l1, l2);
  check_apply(table, {accum, linear}, acc, stamp, ids, epoch);
  check_deep_grad(table, ids, grad);
  emb_bwd_dense(acc, ids, grad, scale);
  launch_apply<FtrlRule>(table, {accum, linear}, acc, stamp, ids, epoch,
                         ftrl_args(lr, l1, l2));
}

void emb_bwd_ftrl_wide(torch::Tensor table, torch::Tensor accum,
                       torch::Tensor linear, torch::Tensor acc,
                       torch::Tensor stamp, torch::Tensor ids,
                       torch::Tensor gw, int64_t epoch, double lr,
                       double l1, double l2, double scale) {
  check_ftrl_args(lr, l1, l2);
  check_apply(table, {accum, linear}, acc, stamp, ids, epoch);
  check_wide_grad(table, ids, gw);
  if (ids.numel() == 0) return;
  emb_scatter_sum(acc, ids, gw, scale);
  launch_apply<FtrlRule>(table, {accum, linear}, acc, stamp, ids, epoch,
                         ftrl_args(lr, l1, l2));
}

// The flagship pair: deep Adagrad + wide FTRL, shared flat ids.
void emb_bwd_adagrad_ftrl_fused_wide(
    torch::Tensor table, torch::Tensor state_sum, torch::Tensor acc,
    torch::Tensor wide_table, torch::Tensor wide_accum,
    torch::Tensor wide_linear, torch::Tensor wide_acc, torch::Tensor stamp,
    torch::Tensor ids, torch::Tensor grad, torch::Tensor gw, int64_t epoch,
    double lr, double eps, double wide_lr, double l1, double l2,
    double scale) {
  check_ftrl_args(wide_lr, l1, l2);
  check_apply_fused_wide(table, {state_sum}, acc, wide_table,
                         {wide_accum, wide_linear}, wide_acc, stamp, ids,
                         epoch);
  check_pair_grads(table, ids, grad, gw);
  emb_bwd_sgd_fused_wide(acc, wide_acc, ids, grad, gw, -1.0, scale);
  launch_apply_fused_wide<AdagradRule, FtrlRule>(
      table, {state_sum}, acc, wide_table, {wide_accum, wide_linear},
      wide_acc, stamp, ids, epoch, adagrad_args(lr, eps),
      ftrl_args(wide_lr, l1, l2));
}

void emb_bwd_ftrl_fused_wide(
    torch::Tensor table, torch::Tensor accum, torch::Tensor linear,
    torch::Tensor acc, torch::Tensor wide_table, torch::Tensor wide_accum,
    torch::Tensor wide_linear, torch::Tensor wide_acc, torch::Tensor stamp,
    torch::Tensor ids, torch::Tensor grad, torch::Tensor gw, int64_t epoch,
    double lr, double wide_lr, double l1, double l2, double scale) {
  check_ftrl_args(lr, l1, l2);
  check_ftrl_args(wide_lr, l1, l2);
  check_apply_fused_wide(table, {accum, linear}, acc, wide_table,
                         {wide_accum, wide_linear}, wide_acc, stamp, ids,
                         epoch);
  check_pair_grads(table, ids, grad, gw);
  emb_bwd_sgd_fused_wide(acc, wide_acc, ids, grad, gw, -1.0, scale);
  launch_apply_fused_wide<FtrlRule, FtrlRule>(
      table, {accum, linear}, acc, wide_table, {wide_accum, wide_linear},
      wide_acc, stamp, ids, epoch, ftrl_args(lr, l1, l2),
      ftrl_args(wide_lr, l1, l2));
}

// Row-wise Adagrad on the unique ids u: G as above, m = sum_c G[u, c]^2 /
// dim, state_row[u] += m, table[u, :] -= lr * G[u, :] / (sqrt(state_row[u])
// + eps).
void emb_bwd_rowwise_adagrad(torch::Tensor table, torch::Tensor state_row,
                             torch::Tensor acc, torch::Tensor stamp,
                             torch::Tensor ids, torch::Tensor grad,
                             int64_t epoch, double lr, double eps,
                             double scale) {
  check_rowwise_apply(table, state_row, acc, stamp, ids, epoch);
  check_deep_grad(table, ids, grad);
  emb_bwd_dense(acc, ids, grad, scale);
  launch_rowwise_apply(table, state_row, acc, stamp, ids, epoch,
                       adagrad_args(lr, eps));
}

// deep row-wise Adagrad + wide Adagrad, shared flat ids
void emb_bwd_rowwise_adagrad_fused_wide(
    torch::Tensor table, torch::Tensor state_row, torch::Tensor acc,
    torch::Tensor wide_table, torch::Tensor wide_state,
    torch::Tensor wide_acc, torch::Tensor stamp, torch::Tensor ids,
    torch::Tensor grad, torch::Tensor gw, int64_t epoch, double lr,
    double eps, double scale) {
  check_rowwise_apply_fused_wide(table, state_row, acc, wide_table,
                                 {wide_state}, wide_acc, stamp, ids, epoch);
  check_pair_grads(table, ids, grad, gw);
  emb_bwd_sgd_fused_wide(acc, wide_acc, ids, grad, gw, -1.0, scale);
  launch_rowwise_apply_fused_wide<AdagradRule>(
      table, state_row, acc, wide_table, {wide_state}, wide_acc, stamp, ids,
      epoch, adagrad_args(lr, eps), adagrad_args(lr, eps));
}

// The recipe with a row-wise deep table: + wide FTRL, shared flat ids.
void emb_bwd_rowwise_adagrad_ftrl_fused_wide(
    torch::Tensor table, torch::Tensor state_row, torch::Tensor acc,
    torch::Tensor wide_table, torch::Tensor wide_accum,
    torch::Tensor wide_linear, torch::Tensor wide_acc, torch::Tensor stamp,
    torch::Tensor ids, torch::Tensor grad, torch::Tensor gw, int64_t epoch,
    double lr, double eps, double wide_lr, double l1, double l2,
    double scale) {
  check_ftrl_args(wide_lr, l1, l2);
  check_rowwise_apply_fused_wide(table, state_row, acc, wide_table,
                                 {wide_accum, wide_linear}, wide_acc, stamp,
                                 ids, epoch);
  check_pair_grads(table, ids, grad, gw);
  emb_bwd_sgd_fused_wide(acc, wide_acc, ids, grad, gw, -1.0, scale);
  launch_rowwise_apply_fused_wide<FtrlRule>(
      table, state_row, acc, wide_table, {wide_accum, wide_linear},
      wide_acc, stamp, ids, epoch, adagrad_args(lr, eps),
      ftrl_args(wide_lr, l1, l2));
}
