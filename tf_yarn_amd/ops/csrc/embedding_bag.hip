// Multi-hot embedding bags for MI355X: pooled lookup from CSR bags and the
// backward that expands pooled gradients into update rows.
//
// A batch of B examples with F features is n_bags = B * F bags; bag
// k = b * F + f holds entries bag_offsets[k] .. bag_offsets[k + 1] - 1 of
// the flat `ids` (and `weights`) arrays, and entry i names table row
// ids[i] + offsets[k % F].
//
//  * emb_bag_fwd:  per bag and column, in fp32,
//        acc = 0;  for i ascending:  acc = acc + row_i[c]           (no weights)
//                                    acc = fmaf(w_i, row_i[c], acc) (weights)
//        out[b, col_offset + f*dim + c] = acc * bag_scale[k]
//    with ONE rounding when `out` is bf16.  bag_scale is 1 ("sum"),
//    1 / len or 1 / sum w ("mean"), 1 / sqrt(len) or 1 / sqrt(sum w^2)
//    ("sqrtn": the fp32 sum, then one rounding of the double
//    1 / sqrt); an empty bag, or a zero denominator, has bag_scale 0 and
//    an all-zero output.  The sum order is ascending position in the bag
//    and nothing else, so a bag gives the same bits wherever it sits.
//  * emb_bag_bwd_rows:  grad_rows[i, c] = g[b, col_offset + f*dim + c] * s_i,
//    s_i = bag_scale[k] (* w_i, one fp32 multiply), rounded to g's dtype:
//    with flat_ids the update list every sparse update op consumes.
//
// Both use emb_fwd_into_kernel's (row, quad) grid-stride map with a bag in
// place of a row: dim/4 consecutive lanes own a bag, each lane one f32x4
// quad, and a lane walks its bag's entries serially.  A bag of thousands
// of entries is therefore one lane group's serial loop: correct, not
// tuned; splitting long bags is not built.  The scalar instantiations
// (one lane per (bag, column)) take the shapes the quads cannot: dim,
// col_offset or a row stride that is no multiple of 4 (the dim-1 wide
// table above all).

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include "common.h"
#include <cstdlib>
#include <string>
#include <vector>

namespace {

enum Combiner { COMB_SUM = 0, COMB_MEAN = 1, COMB_SQRTN = 2 };

// 1 / denominator, 0 where it is 0.  "mean" is one correctly rounded fp32
// division.  "sqrtn" goes through double and rounds once: an fp32 square
// root followed by an fp32 division is off by up to 1.38 ulp (den = 263),
// past the 1 ulp the scale is allowed.  Once per bag, outside the entry
// loop; the CPU path does the same in torch and gets the same bits.
__device__ __forceinline__ float bag_scale_from(float den, int64_t len,
                                                int combiner) {
  if (len == 0) return 0.f;
  if (combiner == COMB_SUM) return 1.f;
  if (den == 0.f) return 0.f;
  if (combiner == COMB_SQRTN) return (float)(1.0 / sqrt((double)den));
  return 1.f / den;
}

// The denominator's next term: every lane of a bag adds the same few
// scalars in the same order, so no shuffle is needed.  w * w + den must
// not contract into an fma: the CPU path rounds the square first.
__device__ __forceinline__ float den_add(float den, float w, int combiner) {
#pragma clang fp contract(off)
  const float term = combiner == COMB_SQRTN ? w * w : w;
  return den + term;
}

template <typename OIo, bool WEIGHTS, bool OFFS>
__global__ void emb_bag_fwd_kernel(
    const float* __restrict__ table, const int64_t* __restrict__ ids,
    const int64_t* __restrict__ bag_offsets,
    const int64_t* __restrict__ offsets, const float* __restrict__ weights,
    typename OIo::scalar_t* __restrict__ out, float* __restrict__ bag_scale,
    int64_t* __restrict__ flat_ids, int64_t n_bags, int64_t dim, int F,
    int64_t out_stride_q, int64_t off_q, int combiner) {
  const int64_t dvec = dim >> 2;
  const int64_t total = n_bags * dvec;
  const int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
       t < total; t += stride) {
    const int64_t k = t / dvec;
    const int64_t c4 = t - k * dvec;
    const int64_t b = k / F;
    const int64_t f = k - b * F;
    const int64_t lo = bag_offsets[k];
    const int64_t hi = bag_offsets[k + 1];
    const int64_t off = OFFS ? offsets[f] : 0;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    float den = WEIGHTS ? 0.f : (float)(hi - lo);
    // loads may run ahead of the adds; the adds keep the entry order
#pragma unroll 4
    for (int64_t i = lo; i < hi; ++i) {
      const int64_t id = ids[i] + off;
      if (OFFS && c4 == 0) flat_ids[i] = id;
      const f32x4 v = reinterpret_cast<const f32x4*>(table + id * dim)[c4];
      if (WEIGHTS) {
        const float w = weights[i];
        den = den_add(den, w, combiner);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = fmaf(w, v[j], acc[j]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __fadd_rn(acc[j], v[j]);
      }
    }
    const float s = bag_scale_from(den, hi - lo, combiner);
    if (combiner != COMB_SUM || s == 0.f) {
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __fmul_rn(acc[j], s);
    }
    QuadIo<OIo>::store4(out, b * out_stride_q + off_q + f * dvec + c4, acc);
    if (c4 == 0) bag_scale[k] = s;
  }
}

// One lane per (bag, column); strides and offsets in elements.
template <typename OIo, bool WEIGHTS, bool OFFS>
__global__ void emb_bag_fwd_scalar_kernel(
    const float* __restrict__ table, const int64_t* __restrict__ ids,
    const int64_t* __restrict__ bag_offsets,
    const int64_t* __restrict__ offsets, const float* __restrict__ weights,
    typename OIo::scalar_t* __restrict__ out, float* __restrict__ bag_scale,
    int64_t* __restrict__ flat_ids, int64_t n_bags, int64_t dim, int F,
    int64_t out_stride, int64_t col_offset, int combiner) {
  const int64_t total = n_bags * dim;
  const int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
       t < total; t += stride) {
    const int64_t k = t / dim;
    const int64_t c = t - k * dim;
    const int64_t b = k / F;
    const int64_t f = k - b * F;
    const int64_t lo = bag_offsets[k];
    const int64_t hi = bag_offsets[k + 1];
    const int64_t off = OFFS ? offsets[f] : 0;
    float acc = 0.f;
    float den = WEIGHTS ? 0.f : (float)(hi - lo);
#pragma unroll 4
    for (int64_t i = lo; i < hi; ++i) {
      const int64_t id = ids[i] + off;
      if (OFFS && c == 0) flat_ids[i] = id;
      const float v = table[id * dim + c];
      if (WEIGHTS) {
        const float w = weights[i];
        den = den_add(den, w, combiner);
        acc = fmaf(w, v, acc);
      } else {
        acc = __fadd_rn(acc, v);
      }
    }
    const float s = bag_scale_from(den, hi - lo, combiner);
    if (combiner != COMB_SUM || s == 0.f) acc = __fmul_rn(acc, s);
    OIo::store(out, b * out_stride + col_offset + f * dim + c, acc);
    if (c == 0) bag_scale[k] = s;
  }
}

template <typename GIo, bool WEIGHTS>
__global__ void emb_bag_bwd_rows_kernel(
    const typename GIo::scalar_t* __restrict__ g,
    const int64_t* __restrict__ bag_offsets,
    const float* __restrict__ bag_scale, const float* __restrict__ weights,
    typename GIo::scalar_t* __restrict__ grad_rows, int64_t n_bags,
    int64_t dim, int F, int64_t g_stride_q, int64_t off_q) {
  const int64_t dvec = dim >> 2;
  const int64_t total = n_bags * dvec;
  const int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
       t < total; t += stride) {
    const int64_t k = t / dvec;
    const int64_t c4 = t - k * dvec;
    const int64_t lo = bag_offsets[k];
    const int64_t hi = bag_offsets[k + 1];
    if (lo >= hi) continue;
    const int64_t b = k / F;
    const int64_t f = k - b * F;
    const float s = bag_scale[k];
    float gq[4];
    QuadIo<GIo>::load4(g, b * g_stride_q + off_q + f * dvec + c4, gq);
    for (int64_t i = lo; i < hi; ++i) {
      const float si = WEIGHTS ? __fmul_rn(s, weights[i]) : s;
      float r[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = __fmul_rn(gq[j], si);
      QuadIo<GIo>::store4(grad_rows, i * dvec + c4, r);
    }
  }
}

template <typename GIo, bool WEIGHTS>
__global__ void emb_bag_bwd_rows_scalar_kernel(
    const typename GIo::scalar_t* __restrict__ g,
    const int64_t* __restrict__ bag_offsets,
    const float* __restrict__ bag_scale, const float* __restrict__ weights,
    typename GIo::scalar_t* __restrict__ grad_rows, int64_t n_bags,
    int64_t dim, int F, int64_t g_stride, int64_t col_offset) {
  const int64_t total = n_bags * dim;
  const int64_t stride = gridDim.x * (int64_t)blockDim.x;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
       t < total; t += stride) {
    const int64_t k = t / dim;
    const int64_t c = t - k * dim;
    const int64_t lo = bag_offsets[k];
    const int64_t hi = bag_offsets[k + 1];
    if (lo >= hi) continue;
    const int64_t b = k / F;
    const int64_t f = k - b * F;
    const float s = bag_scale[k];
    const float gv = GIo::load(g, b * g_stride + col_offset + f * dim + c);
    for (int64_t i = lo; i < hi; ++i) {
      const float si = WEIGHTS ? __fmul_rn(s, weights[i]) : s;
      GIo::store(grad_rows, i * dim + c, __fmul_rn(gv, si));
    }
  }
}

bool bag_bounds_debug_enabled() {
  static const bool on = [] {
    const char* v = std::getenv("MIYARN_DEBUG_BOUNDS");
    return v != nullptr && v[0] != '\0' && v[0] != '0';
  }();
  return on;
}

int parse_combiner(const std::string& combiner) {
  if (combiner == "sum") return COMB_SUM;
  if (combiner == "mean") return COMB_MEAN;
  TORCH_CHECK(combiner == "sqrtn",
              "combiner must be \"sum\", \"mean\" or \"sqrtn\", got \"",
              combiner, "\"");
  return COMB_SQRTN;
}

void check_i64(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
              t.scalar_type() == torch::kInt64,
              name, " must be contiguous int64 on GPU");
}

void check_f32(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
              t.scalar_type() == torch::kFloat32,
              name, " must be a contiguous fp32 GPU tensor");
}

// bag_offsets [n_bags + 1] with n_bags a multiple of F; returns n_bags.
int64_t check_bags(const torch::Tensor& bag_offsets, int64_t n_features,
                   int64_t batch) {
  check_i64(bag_offsets, "bag_offsets");
  TORCH_CHECK(n_features >= 1 && n_features < (int64_t(1) << 31),
              "n_features must be >= 1");
  const int64_t n_bags = batch * n_features;
  TORCH_CHECK(bag_offsets.numel() == n_bags + 1,
              "bag_offsets must have n_bags + 1 = ", n_bags + 1,
              " entries (", batch, " rows x ", n_features,
              " features), got ", bag_offsets.numel());
  return n_bags;
}

// MIYARN_DEBUG_BOUNDS only: waits for the device.
void debug_check_bag_offsets(const torch::Tensor& bag_offsets, int64_t nnz) {
  if (!bag_bounds_debug_enabled()) return;
  const int64_t n = bag_offsets.numel();
  const int64_t first = bag_offsets[0].item<int64_t>();
  const int64_t last = bag_offsets[n - 1].item<int64_t>();
  TORCH_CHECK(first == 0 && last == nnz,
              "bag_offsets must start at 0 and end at nnz = ", nnz,
              ", got [", first, " .. ", last,
              "] (MIYARN_DEBUG_BOUNDS check)");
  if (n > 1) {
    const int64_t step =
        (bag_offsets.slice(0, 1, n) - bag_offsets.slice(0, 0, n - 1))
            .min().item<int64_t>();
    TORCH_CHECK(step >= 0, "bag_offsets must be non-decreasing "
                           "(MIYARN_DEBUG_BOUNDS check)");
  }
}

}  // namespace

// out[b, col_offset + f*dim : +dim] = pooled bag (b, f); returns
// {bag_scale [n_bags] fp32, flat_ids [nnz]} (flat_ids is `ids` itself
// without offsets).
std::vector<torch::Tensor> emb_bag_fwd(
    torch::Tensor table, torch::Tensor ids, torch::Tensor bag_offsets,
    int64_t n_features, c10::optional<torch::Tensor> offsets,
    c10::optional<torch::Tensor> weights, const std::string& combiner,
    torch::Tensor out, int64_t col_offset) {
  check_f32(table, "table");
  TORCH_CHECK(table.dim() == 2 && table.size(1) >= 1,
              "table must be [rows, dim]");
  check_i64(ids, "ids");
  const int comb = parse_combiner(combiner);
  const int64_t dim = table.size(1);
  const int64_t nnz = ids.numel();
  TORCH_CHECK(out.is_cuda() && out.is_contiguous() && out.dim() == 2,
              "out must be a contiguous 2D GPU tensor");
  TORCH_CHECK(out.scalar_type() == torch::kBFloat16 ||
              out.scalar_type() == torch::kFloat32, "out: fp32/bf16 only");
  const int64_t n_bags = check_bags(bag_offsets, n_features, out.size(0));
  TORCH_CHECK(col_offset >= 0 &&
              col_offset + n_features * dim <= out.size(1),
              "slice out of range");
  if (offsets.has_value()) {
    check_i64(*offsets, "offsets");
    TORCH_CHECK(offsets->numel() == n_features,
                "offsets must be int64 [n_features]");
  }
  if (weights.has_value()) {
    check_f32(*weights, "weights");
    TORCH_CHECK(weights->numel() == nnz,
                "weights must have one entry per id: ", nnz, ", got ",
                weights->numel());
  }
  auto bag_scale = torch::empty({n_bags},
                                table.options().dtype(torch::kFloat32));
  auto flat_ids = offsets.has_value() ? torch::empty_like(ids) : ids;
  if (n_bags == 0) return {bag_scale, flat_ids};
  debug_check_bag_offsets(bag_offsets, nnz);
  if (bag_bounds_debug_enabled() && nnz > 0) {
    torch::Tensor flat = ids.reshape({-1});
    if (offsets.has_value()) {
      auto lens = bag_offsets.slice(0, 1, n_bags + 1) -
                  bag_offsets.slice(0, 0, n_bags);
      auto feat = torch::arange(n_bags, ids.options())
                      .remainder(n_features);
      flat = flat + torch::repeat_interleave(
                        offsets->index_select(0, feat), lens);
    }
    const int64_t mn = flat.min().item<int64_t>();
    const int64_t mx = flat.max().item<int64_t>();
    TORCH_CHECK(mn >= 0 && mx < table.size(0),
                "embedding ids out of range: [", mn, ", ", mx,
                "] vs table rows ", table.size(0),
                " (MIYARN_DEBUG_BOUNDS check)");
  }
  const bool bf16 = out.scalar_type() == torch::kBFloat16;
  const bool vec = dim % 4 == 0 && col_offset % 4 == 0 &&
                   out.size(1) % 4 == 0 &&
                   miyarn_aligned(table.data_ptr(), 16) &&
                   miyarn_aligned(out.data_ptr(), bf16 ? 8 : 16);
  const int grid = miyarn_grid(n_bags * (vec ? dim / 4 : dim));
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const int64_t* offs_p =
      offsets.has_value() ? offsets->data_ptr<int64_t>() : nullptr;
  const float* w_p = weights.has_value() ? weights->data_ptr<float>()
                                         : nullptr;
  auto launch = [&](auto io, auto has_w, auto has_o) {
    using Io = decltype(io);
    using S = typename Io::scalar_t;
    constexpr bool W = decltype(has_w)::value;
    constexpr bool O = decltype(has_o)::value;
    if (vec)
      hipLaunchKernelGGL((emb_bag_fwd_kernel<Io, W, O>), dim3(grid),
                         dim3(MIYARN_BLOCK), 0, stream,
                         table.data_ptr<float>(), ids.data_ptr<int64_t>(),
                         bag_offsets.data_ptr<int64_t>(), offs_p, w_p,
                         reinterpret_cast<S*>(out.data_ptr()),
                         bag_scale.data_ptr<float>(),
                         flat_ids.data_ptr<int64_t>(), n_bags, dim,
                         (int)n_features, out.size(1) / 4, col_offset / 4,
                         comb);
    else
      hipLaunchKernelGGL((emb_bag_fwd_scalar_kernel<Io, W, O>), dim3(grid),
                         dim3(MIYARN_BLOCK), 0, stream,
                         table.data_ptr<float>(), ids.data_ptr<int64_t>(),
                         bag_offsets.data_ptr<int64_t>(), offs_p, w_p,
                         reinterpret_cast<S*>(out.data_ptr()),
                         bag_scale.data_ptr<float>(),
                         flat_ids.data_ptr<int64_t>(), n_bags, dim,
                         (int)n_features, out.size(1), col_offset, comb);
  };
  auto with_io = [&](auto io) {
    using T = std::true_type;
    using N = std::false_type;
    if (weights.has_value()) {
      if (offsets.has_value()) launch(io, T{}, T{});
      else launch(io, T{}, N{});
    } else {
      if (offsets.has_value()) launch(io, N{}, T{});
      else launch(io, N{}, N{});
    }
  };
  if (bf16)
    with_io(Bf16Io{});
  else
    with_io(F32Io{});
  return {bag_scale, flat_ids};
}

// grad_rows [nnz, dim] in grad_out's dtype from the whole [B, cols]
// gradient (rows may lie a stride apart), read in place at col_offset.
torch::Tensor emb_bag_bwd_rows(torch::Tensor grad_out,
                               torch::Tensor bag_offsets,
                               torch::Tensor bag_scale, int64_t dim,
                               int64_t n_features, int64_t nnz,
                               c10::optional<torch::Tensor> weights,
                               int64_t col_offset) {
  TORCH_CHECK(grad_out.is_cuda() && grad_out.dim() == 2 &&
              (grad_out.size(1) <= 1 || grad_out.stride(1) == 1) &&
              (grad_out.size(0) <= 1 ||
               grad_out.stride(0) >= grad_out.size(1)),
              "grad_out must be a [B, cols] GPU tensor with unit column "
              "stride");
  TORCH_CHECK(grad_out.scalar_type() == torch::kBFloat16 ||
              grad_out.scalar_type() == torch::kFloat32,
              "grad_out: fp32/bf16 only");
  TORCH_CHECK(dim >= 1 && nnz >= 0, "dim must be >= 1");
  const int64_t n_bags = check_bags(bag_offsets, n_features,
                                    grad_out.size(0));
  check_f32(bag_scale, "bag_scale");
  TORCH_CHECK(bag_scale.numel() == n_bags,
              "bag_scale must have one entry per bag");
  TORCH_CHECK(col_offset >= 0 &&
              col_offset + n_features * dim <= grad_out.size(1),
              "slice out of range");
  if (weights.has_value()) {
    check_f32(*weights, "weights");
    TORCH_CHECK(weights->numel() == nnz,
                "weights must have one entry per id: ", nnz, ", got ",
                weights->numel());
  }
  auto grad_rows = torch::empty({nnz, dim}, grad_out.options());
  if (nnz == 0 || n_bags == 0) return grad_rows;
  debug_check_bag_offsets(bag_offsets, nnz);
  const bool bf16 = grad_out.scalar_type() == torch::kBFloat16;
  const int64_t g_stride =
      grad_out.size(0) > 1 ? grad_out.stride(0) : grad_out.size(1);
  const bool vec = dim % 4 == 0 && col_offset % 4 == 0 &&
                   g_stride % 4 == 0 &&
                   miyarn_aligned(grad_out.data_ptr(), bf16 ? 8 : 16);
  const int grid = miyarn_grid(n_bags * (vec ? dim / 4 : dim));
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const float* w_p = weights.has_value() ? weights->data_ptr<float>()
                                         : nullptr;
  auto launch = [&](auto io, auto has_w) {
    using Io = decltype(io);
    using S = typename Io::scalar_t;
    constexpr bool W = decltype(has_w)::value;
    if (vec)
      hipLaunchKernelGGL((emb_bag_bwd_rows_kernel<Io, W>), dim3(grid),
                         dim3(MIYARN_BLOCK), 0, stream,
                         reinterpret_cast<const S*>(grad_out.data_ptr()),
                         bag_offsets.data_ptr<int64_t>(),
                         bag_scale.data_ptr<float>(), w_p,
                         reinterpret_cast<S*>(grad_rows.data_ptr()), n_bags,
                         dim, (int)n_features, g_stride / 4, col_offset / 4);
    else
      hipLaunchKernelGGL((emb_bag_bwd_rows_scalar_kernel<Io, W>),
                         dim3(grid), dim3(MIYARN_BLOCK), 0, stream,
                         reinterpret_cast<const S*>(grad_out.data_ptr()),
                         bag_offsets.data_ptr<int64_t>(),
                         bag_scale.data_ptr<float>(), w_p,
                         reinterpret_cast<S*>(grad_rows.data_ptr()), n_bags,
                         dim, (int)n_features, g_stride, col_offset);
  };
  auto with_io = [&](auto io) {
    if (weights.has_value()) launch(io, std::true_type{});
    else launch(io, std::false_type{});
  };
  if (bf16)
    with_io(Bf16Io{});
  else
    with_io(F32Io{});
  return grad_rows;
}
