// Stateful sparse optimizers for the embedding tables (Adagrad, FTRL, lazy
// Adam, row-wise Adagrad): accumulate, then claim.
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
// AdagradRule (1 state), FtrlRule and AdamRule (2 states each) are
// instantiated.  That interface is per ELEMENT with table-shaped states: lazy
// Adam is one more such struct, its line in kRules and one line in kDispatch
// per pair wanted; row-wise Adagrad is not.  What lazy Adam adds on the host
// is its scalars: two betas and the table's step count t, which changes with
// every update, so a lazy_adam side carries three more elements (SideArg12)
// and the host folds them, in double, into step_size and the two (1 - beta).
//
// Entry points: emb_bwd_sparse, the one update entry (a deep side, a wide
// side or both; with gradients pass 1 + pass 2, without them pass 2 alone),
// and sparse_pair_fused_ok, which answers from the same kDispatch table
// whether a (deep rule, wide rule, dim) has a fused deep+wide kernel.
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
#include <cmath>
#include <string>
#include <tuple>
#include <type_traits>
#include <variant>
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

// Lazy Adam (torch.optim.SparseAdam on a coalesced gradient, TF LazyAdam);
// s[0] = m (exp_avg), s[1] = v (exp_avg_sq):
//   m' = m + (1 - beta1) * (g - m);  v' = v + (1 - beta2) * (g*g - v);
//   w' = w - step_size * m' / (sqrt(v') + eps),
//   step_size = lr * sqrt(1 - beta2^t) / (1 - beta1^t), formed on the host.
// eps sits outside the root and is not divided by the bias correction (the
// dense fused_adam has torch.optim.Adam's form instead).  The multiply-adds
// are written out (fmaf; the products that must round on their own as
// __fmul_rn), so the quad kernel and the one-lane-per-row kernel give the
// same bits for the same element whatever the compiler would contract.
// One true division, one sqrtf, no clamp: sqrt(v') + eps == 0 needs
// eps == 0 and v' == 0 (a fresh row whose gradient sums to 0), where the
// quotient is 0/0 = NaN exactly as in torch; eps > 0 is the caller's guard.
struct AdamRule {
  struct Args { float step_size, eps, omb1, omb2; };
  static constexpr int kStates = 2;  // exp_avg, exp_avg_sq
  __device__ static __forceinline__ void one(float g, float (&s)[2],
                                             float* w, Args a) {
    const float m = fmaf(a.omb1, g - s[0], s[0]);
    const float v = fmaf(a.omb2, __fmul_rn(g, g) - s[1], s[1]);
    s[0] = m;
    s[1] = v;
    *w -= __fmul_rn(a.step_size, m) / (sqrtf(v) + a.eps);
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

// ---- host: one table's side of an update ------------------------------------

using Tensors = std::vector<torch::Tensor>;

enum RuleId { kAdagrad, kFtrl, kRowwiseAdagrad, kLazyAdam, kNoRule };

// What the host knows about a rule: its name, how many state tensors it
// takes, and whether a state holds one value per table row ([rows], row-wise
// Adagrad) instead of being shaped like the table.
struct RuleInfo {
  const char* name;
  RuleId id;
  size_t n_states;
  bool row_state;
};

const RuleInfo kRules[] = {
    {"adagrad", kAdagrad, 1, false},
    {"ftrl", kFtrl, 2, false},
    {"rowwise_adagrad", kRowwiseAdagrad, 1, true},
    {"lazy_adam", kLazyAdam, 2, false},
};

const RuleInfo& rule_named(const std::string& name) {
  for (const auto& r : kRules)
    if (name == r.name) return r;
  TORCH_CHECK(false, "unknown sparse rule '", name, "'");
  return kRules[0];
}

// A side as the entry point takes it: (rule name, table, the rule's state
// tensors in the rule's order, accumulator, gradient or None, lr, eps, l1,
// l2).  A rule reads the scalars it has and ignores the others.  A lazy_adam
// side, and only that, carries three more: beta1, beta2 and the step count t
// of the update being applied (the first one is t = 1).
using SideArg9 = std::tuple<std::string, torch::Tensor, Tensors,
                            torch::Tensor, c10::optional<torch::Tensor>,
                            double, double, double, double>;
using SideArg12 = std::tuple<std::string, torch::Tensor, Tensors,
                             torch::Tensor, c10::optional<torch::Tensor>,
                             double, double, double, double, double, double,
                             int64_t>;
using SideArg = std::variant<SideArg9, SideArg12>;

struct Side {
  const RuleInfo* rule;
  torch::Tensor table;
  Tensors states;
  torch::Tensor acc;
  c10::optional<torch::Tensor> grad;
  double lr, eps, l1, l2;
  double beta1 = 0.0, beta2 = 0.0;  // lazy_adam only
  int64_t step = 0;
};

Side unpack(const SideArg& arg) {
  if (const auto* a9 = std::get_if<SideArg9>(&arg)) {
    const auto& [rule, table, states, acc, grad, lr, eps, l1, l2] = *a9;
    const RuleInfo& info = rule_named(rule);
    TORCH_CHECK(info.id != kLazyAdam, "a lazy_adam side takes 12 elements: "
                "beta1, beta2 and step after l2");
    return {&info, table, states, acc, grad, lr, eps, l1, l2};
  }
  const auto& [rule, table, states, acc, grad, lr, eps, l1, l2, beta1, beta2,
               step] = std::get<SideArg12>(arg);
  const RuleInfo& info = rule_named(rule);
  TORCH_CHECK(info.id == kLazyAdam, "only a lazy_adam side takes beta1, "
              "beta2 and step; '", info.name, "' takes 9 elements");
  return {&info, table, states, acc, grad, lr, eps, l1, l2, beta1, beta2,
          step};
}

// ---- host: checks -----------------------------------------------------------

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

void check_adam_args(double lr, double eps, double beta1, double beta2,
                     int64_t step) {
  TORCH_CHECK(lr > 0.0, "lazy Adam needs lr > 0");
  TORCH_CHECK(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0,
              "lazy Adam needs 0 <= beta < 1 for both betas");
  TORCH_CHECK(eps >= 0.0, "lazy Adam needs eps >= 0");
  TORCH_CHECK(step >= 1, "lazy Adam needs step >= 1 (the count of updates "
              "applied to the table, this one included)");
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

// One side's scalars, table, states and accumulator.  deep_rows < 0: the
// table whose rows are claimed (2D, any dim); otherwise the wide companion
// of a deep table with that many rows.
void check_side(const Side& s, int64_t deep_rows) {
  const bool companion = deep_rows >= 0;
  if (s.rule->id == kFtrl) check_ftrl_args(s.lr, s.l1, s.l2);
  if (s.rule->id == kLazyAdam)
    check_adam_args(s.lr, s.eps, s.beta1, s.beta2, s.step);
  if (companion) {
    TORCH_CHECK(s.table.is_cuda() && s.table.is_contiguous() &&
                s.table.scalar_type() == torch::kFloat32 &&
                s.table.numel() == deep_rows, "bad wide table");
  } else {
    TORCH_CHECK(s.table.is_cuda() && s.table.is_contiguous() &&
                s.table.dim() == 2 &&
                s.table.scalar_type() == torch::kFloat32,
                "table must be a contiguous 2D fp32 GPU tensor");
  }
  TORCH_CHECK(s.states.size() == s.rule->n_states, s.rule->name, " takes ",
              s.rule->n_states, " state tensor(s), got ", s.states.size());
  for (const auto& st : s.states) {
    if (s.rule->row_state) check_row_state(st, s.table);
    else check_f32_like(st, s.table, companion ? "wide state" : "state");
  }
  check_f32_like(s.acc, s.table, companion ? "wide_acc" : "acc");
}

void check_claim(const torch::Tensor& stamp, const torch::Tensor& ids,
                 int64_t epoch, int64_t rows) {
  TORCH_CHECK(stamp.is_cuda() && stamp.is_contiguous() &&
              stamp.scalar_type() == torch::kInt32 &&
              stamp.numel() == rows,
              "stamp must be contiguous int32 on GPU, one per table row");
  TORCH_CHECK(ids.is_cuda() && ids.is_contiguous() &&
              ids.scalar_type() == torch::kInt64,
              "ids must be contiguous int64 on GPU");
  TORCH_CHECK(epoch >= 1 && epoch < INT32_MAX,
              "epoch must be in [1, 2^31 - 1)");
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

// ---- host: pass-2 launches (inputs already checked) -------------------------

template <int N> StatePtrs<N> state_ptrs(const Tensors& states) {
  StatePtrs<N> p{};
  for (int k = 0; k < N; ++k) p.p[k] = states[k].data_ptr<float>();
  return p;
}

AdagradRule::Args adagrad_args(double lr, double eps) {
  return {(float)lr, (float)eps};
}

FtrlRule::Args ftrl_args(double lr, double l1, double l2) {
  return {(float)lr, (float)l1, (float)l2};
}

// Formed in double and rounded once: 1.f - (float)beta would carry the
// rounding error of beta into a number a hundred times smaller.
AdamRule::Args adam_args(double lr, double eps, double beta1, double beta2,
                         int64_t step) {
  const double bc1 = 1.0 - std::pow(beta1, (double)step);
  const double bc2 = 1.0 - std::pow(beta2, (double)step);
  return {(float)(lr * std::sqrt(bc2) / bc1), (float)eps,
          (float)(1.0 - beta1), (float)(1.0 - beta2)};
}

template <typename Rule> typename Rule::Args rule_args(const Side& s);
template <> AdagradRule::Args rule_args<AdagradRule>(const Side& s) {
  return adagrad_args(s.lr, s.eps);
}
template <> FtrlRule::Args rule_args<FtrlRule>(const Side& s) {
  return ftrl_args(s.lr, s.l1, s.l2);
}

template <> AdamRule::Args rule_args<AdamRule>(const Side& s) {
  return adam_args(s.lr, s.eps, s.beta1, s.beta2, s.step);
}

// The wide companion's kernel arguments; all null under NoRule.
template <typename WideRule> struct WideArgs {
  float* table = nullptr;
  StatePtrs<WideRule::kStates> state{};
  float* acc = nullptr;
  typename WideRule::Args a{};
};

template <typename WideRule> WideArgs<WideRule> wide_args(const Side* w) {
  WideArgs<WideRule> out;
  if constexpr (WideRule::kStates > 0) {
    out.table = w->table.data_ptr<float>();
    out.state = state_ptrs<WideRule::kStates>(w->states);
    out.acc = w->acc.data_ptr<float>();
    out.a = rule_args<WideRule>(*w);
  }
  return out;
}

// An element-wise rule on `d`, with the wide companion `w` under WideRule
// (NoRule: w == nullptr, and dims off the quad map take the row kernel).
template <typename Rule, typename WideRule>
void launch_elementwise(const Side& d, const Side* w,
                        const torch::Tensor& stamp, const torch::Tensor& ids,
                        int64_t epoch) {
  const int64_t dim = d.table.size(1);
  const int64_t n = ids.numel();
  if (n == 0) return;
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const auto st = state_ptrs<Rule::kStates>(d.states);
  const auto a = rule_args<Rule>(d);
  const int shift = quad_shift(dim);
  if (shift >= 0) {
    const auto wd = wide_args<WideRule>(w);
    int grid = miyarn_grid_cap(n << shift, 8192);
    hipLaunchKernelGGL((sparse_adagrad_apply_kernel<Rule, WideRule>),
                       dim3(grid), dim3(MIYARN_BLOCK), 0, stream,
                       d.table.data_ptr<float>(), st,
                       d.acc.data_ptr<float>(), wd.table, wd.state, wd.acc,
                       stamp.data_ptr<int>(), ids.data_ptr<int64_t>(), n,
                       shift, (int)epoch, a, wd.a);
  } else if constexpr (std::is_same_v<WideRule, NoRule>) {
    int grid = miyarn_grid_cap(n, 8192);
    hipLaunchKernelGGL(sparse_adagrad_apply_row_kernel<Rule>, dim3(grid),
                       dim3(MIYARN_BLOCK), 0, stream,
                       d.table.data_ptr<float>(), st,
                       d.acc.data_ptr<float>(), stamp.data_ptr<int>(),
                       ids.data_ptr<int64_t>(), n, dim, (int)epoch, a);
  } else {
    TORCH_INTERNAL_ASSERT(false, "pair at a dim off the quad map");
  }
}

// Row-wise Adagrad on `d`, companion as above.
template <typename WideRule>
void launch_rowwise(const Side& d, const Side* w, const torch::Tensor& stamp,
                    const torch::Tensor& ids, int64_t epoch) {
  const int64_t dim = d.table.size(1);
  const int64_t n = ids.numel();
  if (n == 0) return;
  auto stream = c10::hip::getCurrentHIPStream().stream();
  float* state_row = d.states[0].data_ptr<float>();
  const auto a = rule_args<AdagradRule>(d);
  const int shift = quad_shift(dim);
  if (shift >= 0) {
    const auto wd = wide_args<WideRule>(w);
    int grid = miyarn_grid_cap(n << shift, 8192);
    hipLaunchKernelGGL(rowwise_adagrad_apply_kernel<WideRule>, dim3(grid),
                       dim3(MIYARN_BLOCK), 0, stream,
                       d.table.data_ptr<float>(), state_row,
                       d.acc.data_ptr<float>(), wd.table, wd.state, wd.acc,
                       stamp.data_ptr<int>(), ids.data_ptr<int64_t>(), n,
                       shift, (int)epoch, a, wd.a);
  } else if constexpr (std::is_same_v<WideRule, NoRule>) {
    int grid = miyarn_grid_cap(n, 8192);
    hipLaunchKernelGGL(rowwise_adagrad_apply_row_kernel, dim3(grid),
                       dim3(MIYARN_BLOCK), 0, stream,
                       d.table.data_ptr<float>(), state_row,
                       d.acc.data_ptr<float>(), stamp.data_ptr<int>(),
                       ids.data_ptr<int64_t>(), n, dim, (int)epoch, a);
  } else {
    TORCH_INTERNAL_ASSERT(false, "pair at a dim off the quad map");
  }
}

// ---- host: the dispatch -----------------------------------------------------

// Every pass-2 instantiation there is, by (deep rule, wide rule); kNoRule:
// one table alone, deep or wide.  A pair that is not listed has no fused
// kernel: the entry point refuses it and sparse_pair_fused_ok says so.
// A new pair is one line here.
struct Dispatch {
  RuleId deep, wide;
  void (*launch)(const Side& d, const Side* w, const torch::Tensor& stamp,
                 const torch::Tensor& ids, int64_t epoch);
};

const Dispatch kDispatch[] = {
    {kAdagrad, kNoRule, launch_elementwise<AdagradRule, NoRule>},
    {kFtrl, kNoRule, launch_elementwise<FtrlRule, NoRule>},
    {kRowwiseAdagrad, kNoRule, launch_rowwise<NoRule>},
    {kAdagrad, kAdagrad, launch_elementwise<AdagradRule, AdagradRule>},
    {kAdagrad, kFtrl, launch_elementwise<AdagradRule, FtrlRule>},
    {kFtrl, kFtrl, launch_elementwise<FtrlRule, FtrlRule>},
    {kRowwiseAdagrad, kAdagrad, launch_rowwise<AdagradRule>},
    {kRowwiseAdagrad, kFtrl, launch_rowwise<FtrlRule>},
    {kLazyAdam, kNoRule, launch_elementwise<AdamRule, NoRule>},
    {kLazyAdam, kLazyAdam, launch_elementwise<AdamRule, AdamRule>},
    {kLazyAdam, kFtrl, launch_elementwise<AdamRule, FtrlRule>},
};

const Dispatch* find_dispatch(RuleId deep, RuleId wide) {
  for (const auto& k : kDispatch)
    if (k.deep == deep && k.wide == wide) return &k;
  return nullptr;
}

}  // namespace

// Whether the (deep, wide) rule pair has a fused deep+wide kernel at this
// deep dim: the pair is in kDispatch and dim/4 is a power of two <= 64.
bool sparse_pair_fused_ok(const std::string& deep_rule,
                          const std::string& wide_rule, int64_t dim) {
  return find_dispatch(rule_named(deep_rule).id, rule_named(wide_rule).id) &&
         quad_shift(dim) >= 0;
}

// The stateful sparse update of one table (deep or wide side alone) or of a
// deep table and its [rows, 1] wide companion from their shared flat ids.
// On the unique ids u, G = scale * sum of the gradient rows; then the side's
// rule, once per row:
//   adagrad          state += G^2, table -= lr * G / (sqrt(state) + eps)
//   ftrl             FtrlRule::one per element on (accum, linear, table)
//   lazy_adam        AdamRule::one per element on (exp_avg, exp_avg_sq, table)
//   rowwise_adagrad  state_row[u] += sum_c G[u, c]^2 / dim,
//                    table[u, :] -= lr * G[u, :] / (sqrt(state_row[u]) + eps)
// The wide gradient is per example, in the gw[i / g_div] layout of
// emb_scatter_sum (g_div = ids.numel() / gw.numel()).  Sides without
// gradients run pass 2 alone: their accumulators already hold G.
// Every input is validated, then pass 1 runs, then pass 2.
void emb_bwd_sparse(c10::optional<SideArg> deep, c10::optional<SideArg> wide,
                    torch::Tensor stamp, torch::Tensor ids, int64_t epoch,
                    double scale) {
  TORCH_CHECK(deep || wide, "emb_bwd_sparse needs a deep or a wide side");
  if (deep && wide) {
    const Side d = unpack(*deep), w = unpack(*wide);
    const Dispatch* k = find_dispatch(d.rule->id, w.rule->id);
    TORCH_CHECK(k, "no fused deep+wide kernel for the pair (", d.rule->name,
                ", ", w.rule->name, ")");
    check_side(d, -1);
    check_claim(stamp, ids, epoch, d.table.size(0));
    check_side(w, d.table.size(0));
    TORCH_CHECK(quad_shift(d.table.size(1)) >= 0,
                "the fused deep+wide apply needs dim/4 to be a power of two "
                "<= 64");
    TORCH_CHECK(d.grad.has_value() == w.grad.has_value(),
                "a pair takes both gradients or neither");
    if (d.grad) {
      check_pair_grads(d.table, ids, *d.grad, *w.grad);
      // lr = -1 turns the fused SGD scatter into acc += scale * g
      emb_bwd_sgd_fused_wide(d.acc, w.acc, ids, *d.grad, *w.grad, -1.0,
                             scale);
    }
    k->launch(d, &w, stamp, ids, epoch);
    return;
  }
  const Side s = unpack(deep ? *deep : *wide);
  check_side(s, -1);
  check_claim(stamp, ids, epoch, s.table.size(0));
  if (s.grad) {
    if (deep) check_deep_grad(s.table, ids, *s.grad);
    else check_wide_grad(s.table, ids, *s.grad);
  }
  if (wide && ids.numel() == 0) return;
  if (s.grad) {
    if (deep) emb_bwd_dense(s.acc, ids, *s.grad, scale);
    else emb_scatter_sum(s.acc, ids, *s.grad, scale);
  }
  find_dispatch(s.rule->id, kNoRule)->launch(s, nullptr, stamp, ids, epoch);
}
