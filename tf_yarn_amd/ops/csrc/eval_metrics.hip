// Streaming binary-classification eval state: one pass over a batch of
// (logit, label) folds it into a small persistent device state from which
// the host derives AUC, PR-AUC, accuracy, precision, recall, mean loss and
// the label / prediction means (tf_yarn_amd/estimator/eval_metrics.py).
//
// State (the wrapper owns the tensors, all zero at start):
//   hist   int64 [2, EVAL_BUCKETS]  score histogram, row 0 negatives,
//                                    row 1 positives; buckets are uniform
//                                    in LOGIT space over [-16, 16)
//   counts int64 [4]                (n_valid, n_nan, tp, fp)
//   sums   fp64  [EVAL_SLOTS, 2]    per grid slot (sum loss, sum sigmoid)
//
// Everything that crosses blocks is an integer atomic (order-free) or a
// plain read-add-store into the block's own sums slot (launches are
// stream-ordered), and the in-block float reduction runs in a fixed order:
// the same sequence of batches gives the same state bit for bit.
//
// The pass is 8 B/example against ~10 transcendental-heavy fp32 ops plus an
// LDS atomic; at eval batch sizes (<= a few 100k examples) it is bound by
// the launch and the 32 KB LDS zero/flush per block, not by HBM, so loads
// stay scalar (one example per lane per trip).

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include "common.h"

#define EVAL_BUCKETS 4096
#define EVAL_SLOTS 256  // maximum grid: one sums slot per block

namespace {

__device__ __forceinline__ bool f32_is_nan(float v) {
  union { float f; unsigned int i; } u;
  u.f = v;
  return (u.i & 0x7fffffffu) > 0x7f800000u;
}

// fixed-order wave sum: lane 0 ends with the total
template <typename T>
__device__ __forceinline__ T wave_sum_down(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
  return v;
}

__device__ __forceinline__ void i64_atomic_add(int64_t* p, int64_t v) {
  atomicAdd(reinterpret_cast<unsigned long long*>(p),
            static_cast<unsigned long long>(v));
}

template <typename Io>
__global__ __launch_bounds__(MIYARN_BLOCK) void binary_eval_update_kernel(
    const typename Io::scalar_t* __restrict__ logits,
    const float* __restrict__ labels,
    int64_t* __restrict__ hist,    // [2 * EVAL_BUCKETS]
    int64_t* __restrict__ counts,  // [4]
    double* __restrict__ sums,     // [EVAL_SLOTS * 2]
    int64_t n) {
  constexpr int kWaves = MIYARN_BLOCK / 64;
  __shared__ int lds_hist[2 * EVAL_BUCKETS];
  __shared__ double lds_f[kWaves][2];
  __shared__ int lds_i[kWaves][4];

  for (int b = threadIdx.x; b < 2 * EVAL_BUCKETS; b += MIYARN_BLOCK)
    lds_hist[b] = 0;
  __syncthreads();

  double loss_sum = 0.0, sig_sum = 0.0;
  int n_valid = 0, n_nan = 0, tp = 0, fp = 0;
  const int64_t stride = gridDim.x * (int64_t)MIYARN_BLOCK;
  for (int64_t i = blockIdx.x * (int64_t)MIYARN_BLOCK + threadIdx.x; i < n;
       i += stride) {
    const float z = Io::load(logits, i);
    const float y = labels[i];
    if (f32_is_nan(z) || f32_is_nan(y)) {
      ++n_nan;
      continue;
    }
    const int pos = y >= 0.5f ? 1 : 0;
    // both constants are powers of two: t is one rounding with or without
    // FMA contraction, so the bucket equals the CPU reference's to the bit
    const float t = (z + 16.0f) * 128.0f;
    int k;
    if (t < 0.0f) k = 0;
    else if (t >= (float)EVAL_BUCKETS) k = EVAL_BUCKETS - 1;
    else k = (int)floorf(t);
    atomicAdd(&lds_hist[pos * EVAL_BUCKETS + k], 1);
    ++n_valid;
    const int hot = z > 0.0f ? 1 : 0;  // TF's p > 0.5
    tp += pos & hot;
    fp += (pos ^ 1) & hot;
    // bce_head_fwd_kernel's stable form
    const float loss = fmaxf(z, 0.f) - z * y + log1pf(expf(-fabsf(z)));
    const float sig = 1.f / (1.f + expf(-z));
    loss_sum += (double)loss;
    sig_sum += (double)sig;
  }

  loss_sum = wave_sum_down(loss_sum);
  sig_sum = wave_sum_down(sig_sum);
  n_valid = wave_sum_down(n_valid);
  n_nan = wave_sum_down(n_nan);
  tp = wave_sum_down(tp);
  fp = wave_sum_down(fp);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    lds_f[wave][0] = loss_sum;
    lds_f[wave][1] = sig_sum;
    lds_i[wave][0] = n_valid;
    lds_i[wave][1] = n_nan;
    lds_i[wave][2] = tp;
    lds_i[wave][3] = fp;
  }
  __syncthreads();  // also orders every LDS histogram add before the flush

  for (int b = threadIdx.x; b < 2 * EVAL_BUCKETS; b += MIYARN_BLOCK) {
    const int c = lds_hist[b];
    if (c != 0) i64_atomic_add(&hist[b], c);
  }
  if (threadIdx.x == 0) {
    double l = lds_f[0][0], s = lds_f[0][1];
    for (int w = 1; w < kWaves; ++w) {
      l += lds_f[w][0];
      s += lds_f[w][1];
    }
    // this block owns slot blockIdx.x; earlier launches have completed
    sums[2 * blockIdx.x + 0] += l;
    sums[2 * blockIdx.x + 1] += s;
  } else if (threadIdx.x < 5) {
    const int c = threadIdx.x - 1;
    int64_t v = 0;
    for (int w = 0; w < kWaves; ++w) v += lds_i[w][c];
    if (v != 0) i64_atomic_add(&counts[c], v);
  }
}

}  // namespace

void binary_eval_update(torch::Tensor logits, torch::Tensor labels,
                        torch::Tensor hist, torch::Tensor counts,
                        torch::Tensor sums) {
  const int64_t n = logits.numel();
  TORCH_CHECK(logits.is_cuda() && logits.is_contiguous(),
              "logits: contiguous GPU tensor");
  TORCH_CHECK(n >= 1 && n < (int64_t(1) << 31), "1 <= n < 2^31, got ", n);
  TORCH_CHECK(labels.is_cuda() && labels.is_contiguous() &&
              labels.numel() == n &&
              labels.scalar_type() == torch::kFloat32,
              "labels: contiguous fp32, one per logit");
  TORCH_CHECK(hist.is_cuda() && hist.is_contiguous() &&
              hist.scalar_type() == torch::kInt64 &&
              hist.numel() == 2 * EVAL_BUCKETS,
              "hist: int64 [2, ", EVAL_BUCKETS, "]");
  TORCH_CHECK(counts.is_cuda() && counts.is_contiguous() &&
              counts.scalar_type() == torch::kInt64 && counts.numel() == 4,
              "counts: int64 [4]");
  TORCH_CHECK(sums.is_cuda() && sums.is_contiguous() &&
              sums.scalar_type() == torch::kFloat64 &&
              sums.numel() == 2 * EVAL_SLOTS,
              "sums: float64 [", EVAL_SLOTS, ", 2]");
  for (const auto& t : {labels, hist, counts, sums})
    TORCH_CHECK(t.device() == logits.device(), "tensors on one device");
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const int grid = miyarn_grid_cap(n, EVAL_SLOTS);
  if (logits.scalar_type() == torch::kFloat32) {
    hipLaunchKernelGGL(binary_eval_update_kernel<F32Io>, dim3(grid),
                       dim3(MIYARN_BLOCK), 0, stream,
                       logits.data_ptr<float>(), labels.data_ptr<float>(),
                       hist.data_ptr<int64_t>(), counts.data_ptr<int64_t>(),
                       sums.data_ptr<double>(), n);
  } else {
    TORCH_CHECK(logits.scalar_type() == torch::kBFloat16,
                "logits: fp32 or bf16");
    hipLaunchKernelGGL(
        binary_eval_update_kernel<Bf16Io>, dim3(grid), dim3(MIYARN_BLOCK),
        0, stream,
        reinterpret_cast<const unsigned short*>(logits.data_ptr()),
        labels.data_ptr<float>(), hist.data_ptr<int64_t>(),
        counts.data_ptr<int64_t>(), sums.data_ptr<double>(), n);
  }
}
