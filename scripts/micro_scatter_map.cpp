// Standalone probe of the atomic scatter's ACCESS SHAPE at the bench shape
// (26 x 1M rows, dim 16, 1,703,936 updates, bf16 gradients):
//
//   quad  one thread per quad of a row, four dword atomics each: a
//         wave-instruction touches 16 rows, one dword in each of four
//         16-byte chunks (the map embedding.hip shipped with)
//   elem  one lane per float, 16 consecutive lanes per row: a
//         wave-instruction adds four whole 64-byte rows
//
// Model under test: float atomics leave L2 as one request per 64-byte
// line a wave-instruction touches, so quad costs 4 requests per row and
// elem costs 1.  Every figure is the median of WINDOWS event-timed
// windows of ITERS launches (min..max in brackets); "G req/s" divides the
// model's request count by the median.
//
//   hipcc -O3 --offload-arch=gfx950 scripts/micro_scatter_map.cpp -o msm
//   ./msm            uniform ids
//   ./msm 1.2        Zipf(1.2) ids
//   ./msm 0 6        uniform ids, launches rotate over 6 (ids, gradient)
//                    sets: 408 MB, more than the last-level cache holds,
//                    so every launch reads its inputs from HBM as a
//                    training step does (one set stays cache-resident)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#define CHECK(x) do { auto e = (x); if (e) { printf("err %d @%d\n", e, __LINE__); exit(1); } } while (0)

typedef __attribute__((ext_vector_type(4))) unsigned short bf16x4;

__device__ __forceinline__ void f32aa(float* p, float v) { unsafeAtomicAdd(p, v); }
__device__ __forceinline__ float bf2f(unsigned short u) {
  union { unsigned int i; float f; } v;
  v.i = (unsigned)u << 16;
  return v.f;
}

constexpr int DIM = 16;
constexpr int F = 26;

template <bool WIDE>
__global__ void quad_kernel(float* table, float* wide, const long* ids,
                            const unsigned short* g,
                            const unsigned short* gw, long n) {
  const long dvec = DIM / 4;
  const long total = n * dvec;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < total;
       t += stride) {
    const long row = t / dvec;
    const long c4 = t - row * dvec;
    const long id = ids[row];
    float* dst = table + id * DIM + c4 * 4;
    bf16x4 x = reinterpret_cast<const bf16x4*>(g)[t];
#pragma unroll
    for (int j = 0; j < 4; ++j) f32aa(dst + j, bf2f(x[j]));
    if (WIDE && c4 == 0) f32aa(wide + id, bf2f(gw[row / F]));
  }
}

// U elements per thread per trip, one grid stride apart, all loads issued
// before the first atomic.  SHFL: the lane holding float 0 reads the id
// and the row's other lanes take it by a wave shuffle.
template <bool WIDE, int U, bool SHFL, bool DIVIDE>
__global__ void elem_kernel(float* table, float* wide, const long* ids,
                            const unsigned short* g,
                            const unsigned short* gw, long n, long dim_rt) {
  const long total = n * DIM;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long t0 = blockIdx.x * (long)blockDim.x + threadIdx.x; t0 < total;
       t0 += stride * U) {
    long id[U];
    float v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long t = t0 + u * stride;
      id[u] = -1;
      if (t < total) {
        const long row = DIVIDE ? t / dim_rt : t >> 4;
        if (SHFL) {
          long mine = (t & (DIM - 1)) == 0 ? ids[row] : 0;
          // a row's 16 lanes sit in one wave (stride % 64 == 0)
          id[u] = __shfl(mine, (threadIdx.x & 63) & ~(DIM - 1));
        } else {
          id[u] = ids[row];
        }
        v[u] = bf2f(g[t]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long t = t0 + u * stride;
      if (id[u] < 0) continue;
      const long row = DIVIDE ? t / dim_rt : t >> 4;
      const long c = DIVIDE ? t - row * dim_rt : t & (DIM - 1);
      f32aa(table + id[u] * DIM + c, v[u]);
      if (WIDE && c == 0) f32aa(wide + id[u], bf2f(gw[row / F]));
    }
  }
}

int main(int argc, char** argv) {
  const double zipf = argc > 1 ? atof(argv[1]) : 0.0;
  const int NBUF = argc > 2 ? atoi(argv[2]) : 1;
  const int ITERS = 20, WINDOWS = 7;
  const long rows_per = 1000000, rows = F * rows_per, batch = 65536;
  const long n = batch * F;
  float *table, *wide; long* ids; unsigned short *g, *gw;
  CHECK(hipMalloc(&table, rows * DIM * 4));
  CHECK(hipMalloc(&wide, rows * 4));
  CHECK(hipMalloc(&ids, NBUF * n * 8));
  CHECK(hipMalloc(&g, NBUF * n * DIM * 2));
  CHECK(hipMalloc(&gw, batch * 2));
  std::vector<long> h_ids(NBUF * n);
  std::mt19937_64 rng(1);
  if (zipf > 1.0) {
    // inverse-CDF Zipf over rows_per ranks, per feature
    std::vector<double> cdf(rows_per);
    double s = 0;
    for (long k = 0; k < rows_per; ++k) { s += std::pow(k + 1.0, -zipf); cdf[k] = s; }
    std::uniform_real_distribution<double> U01(0.0, s);
    for (long i = 0; i < NBUF * n; ++i) {
      long k = std::lower_bound(cdf.begin(), cdf.end(), U01(rng)) - cdf.begin();
      h_ids[i] = (i % F) * rows_per + std::min(k, rows_per - 1);
    }
  } else {
    for (long i = 0; i < NBUF * n; ++i) h_ids[i] = (i % F) * rows_per + rng() % rows_per;
  }
  CHECK(hipMemcpy(ids, h_ids.data(), NBUF * n * 8, hipMemcpyHostToDevice));
  CHECK(hipMemset(table, 0, rows * DIM * 4));
  CHECK(hipMemset(wide, 0, rows * 4));
  CHECK(hipMemset(g, 0x3f, NBUF * n * DIM * 2));
  CHECK(hipMemset(gw, 0x3f, batch * 2));
  printf("ids: %s, %ld updates, dim %d, %d input set(s)\n", zipf > 1.0 ? argv[1] : "uniform", n, DIM, NBUF);
  printf("%-34s %6s %9s %21s %9s\n", "map", "grid", "us", "[min..max]", "G req/s");

  auto bench = [&](auto kern, const char* name, long items, int cap,
                   double requests, auto... extra) {
    long blocks = (items + 255) / 256;
    if (blocks > cap) blocks = cap;
    dim3 grid((unsigned)blocks), block(256);
    int k = 0;  // launch counter: picks the input set
    auto launch = [&]() {
      const long b = k++ % NBUF;
      hipLaunchKernelGGL(kern, grid, block, 0, 0, table, wide, ids + b * n,
                         g + b * n * DIM, gw, n, extra...);
    };
    for (int i = 0; i < 3; ++i) launch();
    CHECK(hipDeviceSynchronize());
    std::vector<double> us;
    hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
    for (int w = 0; w < WINDOWS; ++w) {
      hipEventRecord(a);
      for (int i = 0; i < ITERS; ++i) launch();
      hipEventRecord(b);
      CHECK(hipDeviceSynchronize());
      float ms; hipEventElapsedTime(&ms, a, b);
      us.push_back(ms * 1000 / ITERS);
    }
    std::sort(us.begin(), us.end());
    const double med = us[WINDOWS / 2];
    printf("%-34s %6ld %9.1f [%8.1f ..%8.1f] %9.2f\n", name, blocks, med,
           us.front(), us.back(), requests / med * 1e-3);
    fflush(stdout);
  };
  const double R = (double)n;  // one request per update row
  const long NQ = n * DIM / 4, NE = n * DIM;
  bench(quad_kernel<false>, "quad deep", NQ, 8192, 4 * R);
  bench(quad_kernel<true>, "quad deep+wide", NQ, 8192, 5 * R);
  bench(elem_kernel<false, 1, false, true>, "elem deep, int64 divide", NE, 8192, R, (long)DIM);
  for (int cap : {2048, 8192, 32768, 1 << 20}) {
    bench(elem_kernel<false, 1, false, false>, "elem deep U=1", NE, cap, R, (long)DIM);
    bench(elem_kernel<false, 4, false, false>, "elem deep U=4", NE, cap, R, (long)DIM);
  }
  bench(elem_kernel<false, 2, false, false>, "elem deep U=2", NE, 8192, R, (long)DIM);
  bench(elem_kernel<false, 8, false, false>, "elem deep U=8", NE, 8192, R, (long)DIM);
  bench(elem_kernel<false, 4, true, false>, "elem deep U=4, id by shuffle", NE, 8192, R, (long)DIM);
  for (int cap : {8192, 32768}) {
    bench(elem_kernel<true, 1, false, false>, "elem deep+wide U=1", NE, cap, 2 * R, (long)DIM);
    bench(elem_kernel<true, 4, false, false>, "elem deep+wide U=4", NE, cap, 2 * R, (long)DIM);
  }
  bench(elem_kernel<true, 4, true, false>, "elem deep+wide U=4, id by shuffle", NE, 8192, 2 * R, (long)DIM);
  return 0;
}
