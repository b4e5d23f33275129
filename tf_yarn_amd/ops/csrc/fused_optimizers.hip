// Fused optimizer update kernels for MI355X (gfx950).
//
// These replace the per-step optimizer apply the reference delegates to TF /
// torch (optimizer-level allreduce hook + server-side
// apply): one kernel per flat tensor (or per reducer bucket), fp32 states,
// grads in fp32 or bf16, with an optional bf16 "compute copy" of the params
// written in the same pass (mixed-precision master-weight training).
//
// All kernels are memory-bound elementwise: 16 B/lane f32x4 vector accesses,
// grid-stride, grid capped at 2048 blocks (guide Appendix B / G11/G13).
//
// The vector loop needs p, the state buffers and the bf16 copy at their
// natural alignment (16 B, 8 B for the copy).  The host passes vec = false
// for a call where one of them is not (a view into a flat buffer at an odd
// element offset); nvec is then 0 and the scalar tail loop, which starts at
// nvec * 4, takes every element.  g is read by scalars either way.

#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <initializer_list>
#include "common.h"

namespace {

struct SgdArgs {
  float lr, momentum, dampening, weight_decay, scale;
  bool nesterov, first_step;
};

template <typename GIo>
__global__ void sgd_kernel(float* __restrict__ p,
                           const typename GIo::scalar_t* __restrict__ g,
                           float* __restrict__ mom,  // may be null
                           unsigned short* __restrict__ p_bf16,  // may be null
                           int64_t n, bool vec, SgdArgs a) {
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t stride = gridDim.x * (int64_t)blockDim.x;
  const int64_t nvec = vec ? n >> 2 : 0;
  for (int64_t i = tid; i < nvec; i += stride) {
    f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
    f32x4 mv;
    if (mom) mv = reinterpret_cast<f32x4*>(mom)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float gv = GIo::load(g, i * 4 + j) * a.scale;
      gv += a.weight_decay * pv[j];
      if (mom) {
        float m = a.first_step ? gv
                               : a.momentum * mv[j] + (1.f - a.dampening) * gv;
        mv[j] = m;
        gv = a.nesterov ? gv + a.momentum * m : m;
      }
      pv[j] -= a.lr * gv;
    }
    reinterpret_cast<f32x4*>(p)[i] = pv;
    if (mom) reinterpret_cast<f32x4*>(mom)[i] = mv;
    if (p_bf16) {
      bf16x4 bv;
#pragma unroll
      for (int j = 0; j < 4; ++j) bv[j] = f32_to_bf16(pv[j]);
      reinterpret_cast<bf16x4*>(p_bf16)[i] = bv;
    }
  }
  for (int64_t i = (nvec << 2) + tid; i < n; i += stride) {
    float pv = p[i];
    float gv = GIo::load(g, i) * a.scale;
    gv += a.weight_decay * pv;
    if (mom) {
      float m = a.first_step ? gv
                             : a.momentum * mom[i] + (1.f - a.dampening) * gv;
      mom[i] = m;
      gv = a.nesterov ? gv + a.momentum * m : m;
    }
    pv -= a.lr * gv;
    p[i] = pv;
    if (p_bf16) p_bf16[i] = f32_to_bf16(pv);
  }
}

// omb1 / omb2 are 1 - beta rounded ONCE from the host's double: 1.f - beta
// in fp32 is exact, but on the already rounded beta, and the rounding error
// of beta = 0.99 is a 1e-6 relative error of 0.01, which put exp_avg_sq 8
// ulps from a float64 evaluation where the CPU path is within 1.2.
struct AdamArgs {
  float lr, beta1, beta2, omb1, omb2, eps, weight_decay, bc1, bc2, scale;
  bool adamw;
};

// One element of Adam / AdamW.  The vector loop and the scalar tail both go
// through this function, and its multiply-adds are written out (fmaf, with
// contraction off for the rest), so an element gets the same roundings
// whichever loop takes it: a misaligned view, which runs the tail loop
// only, gives the bits of an aligned one.
__device__ __forceinline__ void adam_one(float g, float* p, float* m,
                                         float* v, AdamArgs a) {
#pragma clang fp contract(off)
  float pv = *p;
  float gv = g * a.scale;
  if (a.adamw) pv = fmaf(-(a.lr * a.weight_decay), pv, pv);
  else gv = fmaf(a.weight_decay, pv, gv);
  const float mm = fmaf(a.beta1, *m, a.omb1 * gv);
  const float vv = fmaf(a.beta2, *v, a.omb2 * gv * gv);
  *m = mm;
  *v = vv;
  *p = pv - a.lr * (mm / a.bc1) / (sqrtf(vv / a.bc2) + a.eps);
}

template <typename GIo>
__global__ void adam_kernel(float* __restrict__ p,
                            const typename GIo::scalar_t* __restrict__ g,
                            float* __restrict__ m_, float* __restrict__ v_,
                            unsigned short* __restrict__ p_bf16,
                            int64_t n, bool vec, AdamArgs a) {
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t stride = gridDim.x * (int64_t)blockDim.x;
  const int64_t nvec = vec ? n >> 2 : 0;
  for (int64_t i = tid; i < nvec; i += stride) {
    f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
    f32x4 mv = reinterpret_cast<f32x4*>(m_)[i];
    f32x4 vv = reinterpret_cast<f32x4*>(v_)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float pp = pv[j], mm = mv[j], v2 = vv[j];
      adam_one(GIo::load(g, i * 4 + j), &pp, &mm, &v2, a);
      pv[j] = pp; mv[j] = mm; vv[j] = v2;
    }
    reinterpret_cast<f32x4*>(p)[i] = pv;
    reinterpret_cast<f32x4*>(m_)[i] = mv;
    reinterpret_cast<f32x4*>(v_)[i] = vv;
    if (p_bf16) {
      bf16x4 bv;
#pragma unroll
      for (int j = 0; j < 4; ++j) bv[j] = f32_to_bf16(pv[j]);
      reinterpret_cast<bf16x4*>(p_bf16)[i] = bv;
    }
  }
  for (int64_t i = (nvec << 2) + tid; i < n; i += stride) {
    float pv = p[i], m = m_[i], v = v_[i];
    adam_one(GIo::load(g, i), &pv, &m, &v, a);
    p[i] = pv; m_[i] = m; v_[i] = v;
    if (p_bf16) p_bf16[i] = f32_to_bf16(pv);
  }
}

struct AdagradArgs { float lr, eps, weight_decay, scale; };

// One element of Adagrad, shared by both loops (see adam_one).
__device__ __forceinline__ void adagrad_one(float g, float* p, float* acc,
                                            AdagradArgs a) {
#pragma clang fp contract(off)
  const float gv = fmaf(a.weight_decay, *p, g * a.scale);
  const float s = fmaf(gv, gv, *acc);
  *acc = s;
  *p -= a.lr * gv / (sqrtf(s) + a.eps);
}

template <typename GIo>
__global__ void adagrad_kernel(float* __restrict__ p,
                               const typename GIo::scalar_t* __restrict__ g,
                               float* __restrict__ acc,
                               int64_t n, bool vec, AdagradArgs a) {
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t stride = gridDim.x * (int64_t)blockDim.x;
  const int64_t nvec = vec ? n >> 2 : 0;
  for (int64_t i = tid; i < nvec; i += stride) {
    f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
    f32x4 av = reinterpret_cast<f32x4*>(acc)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float pp = pv[j], aa = av[j];
      adagrad_one(GIo::load(g, i * 4 + j), &pp, &aa, a);
      pv[j] = pp; av[j] = aa;
    }
    reinterpret_cast<f32x4*>(p)[i] = pv;
    reinterpret_cast<f32x4*>(acc)[i] = av;
  }
  for (int64_t i = (nvec << 2) + tid; i < n; i += stride)
    adagrad_one(GIo::load(g, i), &p[i], &acc[i], a);
}

// Dense FTRL-proximal (TF Ftrl, learning_rate_power = -0.5, no beta, no L2
// shrinkage): every element is recomputed from (z, n) every step.  The
// rule is the one of the sparse tables (sparse_adagrad.hip, FtrlRule); q
// can only be 0 where n' == 0 and l2 == 0, and there |z'| > l1 is false
// for any state the rule itself produced, so the division is never reached.
struct FtrlArgs { float lr, l1, l2, scale; };

__device__ __forceinline__ void ftrl_one(float g, float* n, float* z,
                                         float* w, FtrlArgs a) {
  const float n_new = *n + g * g;
  const float r_new = sqrtf(n_new);
  const float zz = *z + g - (r_new - sqrtf(*n)) / a.lr * *w;
  const float q = r_new / a.lr + 2.f * a.l2;
  *n = n_new;
  *z = zz;
  *w = fabsf(zz) > a.l1 ? (copysignf(a.l1, zz) - zz) / q : 0.f;
}

template <typename GIo>
__global__ void ftrl_kernel(float* __restrict__ p,
                            const typename GIo::scalar_t* __restrict__ g,
                            float* __restrict__ accum,
                            float* __restrict__ linear,
                            int64_t n, bool vec, FtrlArgs a) {
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t stride = gridDim.x * (int64_t)blockDim.x;
  const int64_t nvec = vec ? n >> 2 : 0;
  for (int64_t i = tid; i < nvec; i += stride) {
    f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
    f32x4 nv = reinterpret_cast<f32x4*>(accum)[i];
    f32x4 zv = reinterpret_cast<f32x4*>(linear)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float nn = nv[j], zz = zv[j], ww = pv[j];
      ftrl_one(GIo::load(g, i * 4 + j) * a.scale, &nn, &zz, &ww, a);
      nv[j] = nn; zv[j] = zz; pv[j] = ww;
    }
    reinterpret_cast<f32x4*>(p)[i] = pv;
    reinterpret_cast<f32x4*>(accum)[i] = nv;
    reinterpret_cast<f32x4*>(linear)[i] = zv;
  }
  for (int64_t i = (nvec << 2) + tid; i < n; i += stride)
    ftrl_one(GIo::load(g, i) * a.scale, &accum[i], &linear[i], &p[i], a);
}

// omr = 1 - rho from the host's double, as omb1 / omb2 above.
struct AdadeltaArgs { float lr, rho, omr, eps, weight_decay, scale; };

// One element of Adadelta, shared by both loops (see adam_one).
__device__ __forceinline__ void adadelta_one(float g, float* p, float* sq,
                                             float* acc_d, AdadeltaArgs a) {
#pragma clang fp contract(off)
  const float gv = fmaf(a.weight_decay, *p, g * a.scale);
  const float s = fmaf(a.rho, *sq, a.omr * gv * gv);
  const float dx = sqrtf(*acc_d + a.eps) / sqrtf(s + a.eps) * gv;
  *sq = s;
  *acc_d = fmaf(a.rho, *acc_d, a.omr * dx * dx);
  *p = fmaf(-a.lr, dx, *p);
}

template <typename GIo>
__global__ void adadelta_kernel(float* __restrict__ p,
                                const typename GIo::scalar_t* __restrict__ g,
                                float* __restrict__ sq,
                                float* __restrict__ acc_d,
                                int64_t n, bool vec, AdadeltaArgs a) {
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t stride = gridDim.x * (int64_t)blockDim.x;
  const int64_t nvec = vec ? n >> 2 : 0;
  for (int64_t i = tid; i < nvec; i += stride) {
    f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
    f32x4 sv = reinterpret_cast<f32x4*>(sq)[i];
    f32x4 dv = reinterpret_cast<f32x4*>(acc_d)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float pp = pv[j], ss = sv[j], dd = dv[j];
      adadelta_one(GIo::load(g, i * 4 + j), &pp, &ss, &dd, a);
      pv[j] = pp; sv[j] = ss; dv[j] = dd;
    }
    reinterpret_cast<f32x4*>(p)[i] = pv;
    reinterpret_cast<f32x4*>(sq)[i] = sv;
    reinterpret_cast<f32x4*>(acc_d)[i] = dv;
  }
  for (int64_t i = (nvec << 2) + tid; i < n; i += stride)
    adadelta_one(GIo::load(g, i), &p[i], &sq[i], &acc_d[i], a);
}

// ---- multi-tensor SGD ------------------------------------------------------
// One launch for all dense params of a group (the per-param launches were
// ~10 x 4.6 us/step in the profile): gridDim.y = tensor index, each y-slice
// grid-strides its own tensor.  Kernel-arg struct holds up to MT_MAX
// tensors (HIP kernarg limit 4 KB).

#define MT_MAX 24

struct MtTensors {
  float* p[MT_MAX];
  const void* g[MT_MAX];
  float* m[MT_MAX];           // nullptr if no momentum
  unsigned short* pb[MT_MAX]; // nullptr if no bf16 copy
  long numel[MT_MAX];
  bool vec[MT_MAX];           // this tensor's pointers are vector-aligned
  int n;
};

template <typename GIo>
__global__ void sgd_mt_kernel(MtTensors t, SgdArgs a) {
  const int ti = blockIdx.y;
  if (ti >= t.n) return;
  const int64_t n = t.numel[ti];
  float* __restrict__ p = t.p[ti];
  const typename GIo::scalar_t* __restrict__ g =
      reinterpret_cast<const typename GIo::scalar_t*>(t.g[ti]);
  float* __restrict__ mom = t.m[ti];
  unsigned short* __restrict__ pb = t.pb[ti];
  const bool vec = t.vec[ti];
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t stride = gridDim.x * (int64_t)blockDim.x;
  const int64_t nvec = vec ? n >> 2 : 0;
  for (int64_t i = tid; i < nvec; i += stride) {
    f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
    f32x4 mv;
    if (mom) mv = reinterpret_cast<f32x4*>(mom)[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float gv = GIo::load(g, i * 4 + j) * a.scale;
      gv += a.weight_decay * pv[j];
      if (mom) {
        float m = a.first_step ? gv
                               : a.momentum * mv[j] + (1.f - a.dampening) * gv;
        mv[j] = m;
        gv = a.nesterov ? gv + a.momentum * m : m;
      }
      pv[j] -= a.lr * gv;
    }
    reinterpret_cast<f32x4*>(p)[i] = pv;
    if (mom) reinterpret_cast<f32x4*>(mom)[i] = mv;
    if (pb) {
      bf16x4 bv;
#pragma unroll
      for (int j = 0; j < 4; ++j) bv[j] = f32_to_bf16(pv[j]);
      reinterpret_cast<bf16x4*>(pb)[i] = bv;
    }
  }
  for (int64_t i = (nvec << 2) + tid; i < n; i += stride) {
    float pv = p[i];
    float gv = GIo::load(g, i) * a.scale;
    gv += a.weight_decay * pv;
    if (mom) {
      float m = a.first_step ? gv
                             : a.momentum * mom[i] + (1.f - a.dampening) * gv;
      mom[i] = m;
      gv = a.nesterov ? gv + a.momentum * m : m;
    }
    pv -= a.lr * gv;
    p[i] = pv;
    if (pb) pb[i] = f32_to_bf16(pv);
  }
}

// ---- host-side checks/dispatch --------------------------------------------

void check_flat_f32(const torch::Tensor& t, const char* name, int64_t n) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, name, " must be fp32");
  TORCH_CHECK(t.numel() == n, name, " numel mismatch");
}

void check_grad(const torch::Tensor& g, int64_t n) {
  TORCH_CHECK(g.is_cuda() && g.is_contiguous(), "grad must be GPU+contig");
  TORCH_CHECK(g.scalar_type() == torch::kFloat32 ||
              g.scalar_type() == torch::kBFloat16,
              "grad must be fp32 or bf16");
  TORCH_CHECK(g.numel() == n, "grad numel mismatch");
}

// True when every vector-accessed pointer of a launch has its alignment:
// f32 (p and the states; null = absent) 16 B, the bf16 copy 8 B.
bool vec_aligned(std::initializer_list<const void*> f32,
                 const void* bf16 = nullptr) {
  for (const void* p : f32)
    if (!miyarn_aligned(p, 16)) return false;
  return miyarn_aligned(bf16, 8);
}

unsigned short* bf16_copy_ptr(const c10::optional<torch::Tensor>& t,
                              int64_t n) {
  if (!t.has_value()) return nullptr;
  TORCH_CHECK(t->is_cuda() && t->is_contiguous() &&
              t->scalar_type() == torch::kBFloat16 && t->numel() == n,
              "param_bf16 must be a contiguous bf16 GPU tensor of same size");
  return reinterpret_cast<unsigned short*>(t->data_ptr());
}

}  // namespace

void fused_sgd(torch::Tensor param, torch::Tensor grad,
               c10::optional<torch::Tensor> momentum_buf,
               c10::optional<torch::Tensor> param_bf16,
               double lr, double momentum, double dampening,
               double weight_decay, bool nesterov, bool first_step,
               double grad_scale) {
  int64_t n = param.numel();
  check_flat_f32(param, "param", n);
  check_grad(grad, n);
  float* mom = nullptr;
  if (momentum_buf.has_value()) {
    check_flat_f32(*momentum_buf, "momentum", n);
    mom = momentum_buf->data_ptr<float>();
  }
  SgdArgs a{(float)lr, (float)momentum, (float)dampening,
            (float)weight_decay, (float)grad_scale, nesterov, first_step};
  auto stream = c10::hip::getCurrentHIPStream().stream();
  int grid = miyarn_grid((n + 3) / 4);
  unsigned short* pb = bf16_copy_ptr(param_bf16, n);
  const bool vec = vec_aligned({param.data_ptr(), mom}, pb);
  if (grad.scalar_type() == torch::kFloat32) {
    hipLaunchKernelGGL(sgd_kernel<F32Io>, dim3(grid), dim3(MIYARN_BLOCK), 0,
                       stream, param.data_ptr<float>(),
                       grad.data_ptr<float>(), mom, pb, n, vec, a);
  } else {
    hipLaunchKernelGGL(sgd_kernel<Bf16Io>, dim3(grid), dim3(MIYARN_BLOCK), 0,
                       stream, param.data_ptr<float>(),
                       reinterpret_cast<unsigned short*>(grad.data_ptr()),
                       mom, pb, n, vec, a);
  }
}

void fused_sgd_mt(std::vector<torch::Tensor> params,
                  std::vector<torch::Tensor> grads,
                  std::vector<torch::Tensor> momentum_bufs,  // may be empty
                  std::vector<torch::Tensor> params_bf16,    // may be empty
                  double lr, double momentum, double dampening,
                  double weight_decay, bool nesterov, bool first_step,
                  double grad_scale) {
  const int n = static_cast<int>(params.size());
  TORCH_CHECK(n > 0 && (int)grads.size() == n, "params/grads mismatch");
  const bool has_mom = !momentum_bufs.empty();
  const bool has_bf16 = !params_bf16.empty();
  TORCH_CHECK(!has_mom || (int)momentum_bufs.size() == n, "momentum size");
  TORCH_CHECK(!has_bf16 || (int)params_bf16.size() == n, "bf16 size");
  auto gtype = grads[0].scalar_type();
  SgdArgs a{(float)lr, (float)momentum, (float)dampening,
            (float)weight_decay, (float)grad_scale, nesterov, first_step};
  auto stream = c10::hip::getCurrentHIPStream().stream();
  for (int base = 0; base < n; base += MT_MAX) {
    MtTensors t{};
    int k = std::min(MT_MAX, n - base);
    t.n = k;
    int64_t max_numel = 0;
    for (int i = 0; i < k; ++i) {
      const auto& p = params[base + i];
      const auto& g = grads[base + i];
      int64_t ne = p.numel();
      check_flat_f32(p, "param", ne);
      check_grad(g, ne);
      TORCH_CHECK(g.scalar_type() == gtype,
                  "all grads in one fused_sgd_mt call share a dtype");
      t.p[i] = p.data_ptr<float>();
      t.g[i] = g.data_ptr();
      t.m[i] = nullptr;
      t.pb[i] = nullptr;
      if (has_mom) {
        check_flat_f32(momentum_bufs[base + i], "momentum", ne);
        t.m[i] = momentum_bufs[base + i].data_ptr<float>();
      }
      if (has_bf16) {
        t.pb[i] = bf16_copy_ptr(
            c10::optional<torch::Tensor>(params_bf16[base + i]), ne);
      }
      t.numel[i] = ne;
      t.vec[i] = vec_aligned({t.p[i], t.m[i]}, t.pb[i]);
      max_numel = std::max(max_numel, ne);
    }
    dim3 grid(miyarn_grid((max_numel + 3) / 4), k);
    if (gtype == torch::kFloat32) {
      hipLaunchKernelGGL(sgd_mt_kernel<F32Io>, grid, dim3(MIYARN_BLOCK), 0,
                         stream, t, a);
    } else {
      hipLaunchKernelGGL(sgd_mt_kernel<Bf16Io>, grid, dim3(MIYARN_BLOCK), 0,
                         stream, t, a);
    }
  }
}

void fused_adam(torch::Tensor param, torch::Tensor grad,
                torch::Tensor exp_avg, torch::Tensor exp_avg_sq,
                c10::optional<torch::Tensor> param_bf16,
                double lr, double beta1, double beta2, double eps,
                double weight_decay, bool adamw, int64_t step,
                double grad_scale) {
  int64_t n = param.numel();
  check_flat_f32(param, "param", n);
  check_flat_f32(exp_avg, "exp_avg", n);
  check_flat_f32(exp_avg_sq, "exp_avg_sq", n);
  check_grad(grad, n);
  AdamArgs a{(float)lr, (float)beta1, (float)beta2,
             (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps,
             (float)weight_decay,
             (float)(1.0 - std::pow(beta1, (double)step)),
             (float)(1.0 - std::pow(beta2, (double)step)),
             (float)grad_scale, adamw};
  auto stream = c10::hip::getCurrentHIPStream().stream();
  int grid = miyarn_grid((n + 3) / 4);
  unsigned short* pb = bf16_copy_ptr(param_bf16, n);
  const bool vec = vec_aligned(
      {param.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr()}, pb);
  if (grad.scalar_type() == torch::kFloat32) {
    hipLaunchKernelGGL(adam_kernel<F32Io>, dim3(grid), dim3(MIYARN_BLOCK), 0,
                       stream, param.data_ptr<float>(),
                       grad.data_ptr<float>(), exp_avg.data_ptr<float>(),
                       exp_avg_sq.data_ptr<float>(),
                       pb, n, vec, a);
  } else {
    hipLaunchKernelGGL(adam_kernel<Bf16Io>, dim3(grid), dim3(MIYARN_BLOCK), 0,
                       stream, param.data_ptr<float>(),
                       reinterpret_cast<unsigned short*>(grad.data_ptr()),
                       exp_avg.data_ptr<float>(),
                       exp_avg_sq.data_ptr<float>(),
                       pb, n, vec, a);
  }
}

void fused_adagrad(torch::Tensor param, torch::Tensor grad,
                   torch::Tensor state_sum, double lr, double eps,
                   double weight_decay, double grad_scale) {
  int64_t n = param.numel();
  check_flat_f32(param, "param", n);
  check_flat_f32(state_sum, "state_sum", n);
  check_grad(grad, n);
  AdagradArgs a{(float)lr, (float)eps, (float)weight_decay,
                (float)grad_scale};
  auto stream = c10::hip::getCurrentHIPStream().stream();
  int grid = miyarn_grid((n + 3) / 4);
  const bool vec = vec_aligned({param.data_ptr(), state_sum.data_ptr()});
  if (grad.scalar_type() == torch::kFloat32) {
    hipLaunchKernelGGL(adagrad_kernel<F32Io>, dim3(grid), dim3(MIYARN_BLOCK),
                       0, stream, param.data_ptr<float>(),
                       grad.data_ptr<float>(), state_sum.data_ptr<float>(),
                       n, vec, a);
  } else {
    hipLaunchKernelGGL(adagrad_kernel<Bf16Io>, dim3(grid), dim3(MIYARN_BLOCK),
                       0, stream, param.data_ptr<float>(),
                       reinterpret_cast<unsigned short*>(grad.data_ptr()),
                       state_sum.data_ptr<float>(), n, vec, a);
  }
}

void fused_ftrl(torch::Tensor param, torch::Tensor grad,
                torch::Tensor accum, torch::Tensor linear, double lr,
                double l1, double l2, double grad_scale) {
  int64_t n = param.numel();
  TORCH_CHECK(lr > 0.0, "FTRL needs lr > 0");
  TORCH_CHECK(l1 >= 0.0 && l2 >= 0.0, "FTRL needs l1 >= 0 and l2 >= 0");
  check_flat_f32(param, "param", n);
  check_flat_f32(accum, "accum", n);
  check_flat_f32(linear, "linear", n);
  check_grad(grad, n);
  FtrlArgs a{(float)lr, (float)l1, (float)l2, (float)grad_scale};
  auto stream = c10::hip::getCurrentHIPStream().stream();
  int grid = miyarn_grid((n + 3) / 4);
  const bool vec = vec_aligned(
      {param.data_ptr(), accum.data_ptr(), linear.data_ptr()});
  if (grad.scalar_type() == torch::kFloat32) {
    hipLaunchKernelGGL(ftrl_kernel<F32Io>, dim3(grid), dim3(MIYARN_BLOCK),
                       0, stream, param.data_ptr<float>(),
                       grad.data_ptr<float>(), accum.data_ptr<float>(),
                       linear.data_ptr<float>(), n, vec, a);
  } else {
    hipLaunchKernelGGL(ftrl_kernel<Bf16Io>, dim3(grid), dim3(MIYARN_BLOCK),
                       0, stream, param.data_ptr<float>(),
                       reinterpret_cast<unsigned short*>(grad.data_ptr()),
                       accum.data_ptr<float>(), linear.data_ptr<float>(),
                       n, vec, a);
  }
}

void fused_adadelta(torch::Tensor param, torch::Tensor grad,
                    torch::Tensor square_avg, torch::Tensor acc_delta,
                    double lr, double rho, double eps, double weight_decay,
                    double grad_scale) {
  int64_t n = param.numel();
  check_flat_f32(param, "param", n);
  check_flat_f32(square_avg, "square_avg", n);
  check_flat_f32(acc_delta, "acc_delta", n);
  check_grad(grad, n);
  AdadeltaArgs a{(float)lr, (float)rho, (float)(1.0 - rho), (float)eps,
                 (float)weight_decay,
                 (float)grad_scale};
  auto stream = c10::hip::getCurrentHIPStream().stream();
  int grid = miyarn_grid((n + 3) / 4);
  const bool vec = vec_aligned(
      {param.data_ptr(), square_avg.data_ptr(), acc_delta.data_ptr()});
  if (grad.scalar_type() == torch::kFloat32) {
    hipLaunchKernelGGL(adadelta_kernel<F32Io>, dim3(grid), dim3(MIYARN_BLOCK),
                       0, stream, param.data_ptr<float>(),
                       grad.data_ptr<float>(), square_avg.data_ptr<float>(),
                       acc_delta.data_ptr<float>(), n, vec, a);
  } else {
    hipLaunchKernelGGL(adadelta_kernel<Bf16Io>, dim3(grid),
                       dim3(MIYARN_BLOCK), 0, stream,
                       param.data_ptr<float>(),
                       reinterpret_cast<unsigned short*>(grad.data_ptr()),
                       square_avg.data_ptr<float>(),
                       acc_delta.data_ptr<float>(), n, vec, a);
  }
}
