// The annotated transformer's LayerNorm as DCP uses it (registration/models/dcp.py: LayerNorm; reference dcp.py:144-154),
// with the residual sum in front of it, forward and backward.  Per row of d values, z = x + delta (or x):
//   mean = sum(z) / d,  c = z - mean,  std = sqrt(sum(c * c) / (d - 1)),  U = 1 / (std + eps),  y = (a * c) * U + b
// -- the UNBIASED std taken from the centred values, eps added to the std: not nn.LayerNorm.  The reference runs it as two
// reductions and four elementwise passes over the (rows, d) tensor, the residual sum as a pass of its own, and autograd
// keeps every intermediate; here a row is read once and written once (twice with the sum), and the backward pass reads z,
// gy (and the residual stream's gradient) once and writes gz once, from z and the row's {mean, std} alone:
//   gh = gy * a,  gz = U * (gh - mean(gh)) - c * (sum(gh * c) * U^2 / ((d - 1) * std))  [+ gres]
//   ga[j] = sum_r gy[r,j] * c[r,j] * U_r,  gb[j] = sum_r gy[r,j]
// (the second term of gz is 0 where std == 0, the value torch's std backward gives a constant row).
//
// One wave per row: d <= 1024 floats are at most four float4 per lane (NV = ceil(d / 256) of them, a template parameter;
// 512 floats = 8 per lane), the row stays in registers between the two passes of the variance.  A lane adds its own values
// in ascending order (at most 15 additions), the 64 partial sums meet in wave_sum's six DPP steps.  Workgroups of four
// waves walk the rows with a grid stride; the grid, ln_grid(rows), depends on the row count alone.
// The backward pass re-centres z on the row's mean taken to double (one more wave sum, of the exact differences
// z - mean): a centred value near the mean then has a relative error of an ulp, which the column sums over few rows need.
// ga / gb: a lane adds its columns over the rows its wave visits (in registers; in the wave's LDS slice at d > 768), the four waves of a workgroup are added in wave order
// through LDS and leave one slab [2][d] in the caller's scratch; ln_slab_sum_kernel adds the slabs in ascending order, 16
// runs of them per column and then the 16 partial sums in order.  No atomics, nothing passes between workgroups inside a
// launch: the same bits on every run.
// Non-finite rows: a NaN or an Inf in a row makes its mean or its centred values NaN, hence std, U and all d entries of y
// and gz; no other row is touched, and a column of ga / gb is NaN if a contributing row is.
// Host side: the guards are common.h's (misaligned, bad_eps, scratch_short), NV is picked once, in MVP_LN_LAUNCH.
#include "common.h"
#include "wave.h"

namespace mvp {

constexpr int kLnThreads = 256;                    // four waves, a row each
constexpr int kLnWaves = kLnThreads / kWave;
constexpr int kLnMaxD = 1024;
constexpr int kLnMaxGrid = 2048;                   // workgroups: 8 per CU of a 256-CU chip, and the number of slabs
constexpr int kLnSumParts = 16;                    // runs of slabs per column in ln_slab_sum_kernel

static inline int ln_grid(int rows) {
  const int need = (rows + kLnWaves - 1) / kLnWaves;
  return need < kLnMaxGrid ? need : kLnMaxGrid;
}

__device__ __forceinline__ float ln_lane_sum(const float4 &v) { return ((v.x + v.y) + v.z) + v.w; }
__device__ __forceinline__ float4 ln_sub(const float4 &v, float m) { return make_float4(v.x - m, v.y - m, v.z - m, v.w - m); }
__device__ __forceinline__ float4 ln_mul(const float4 &p, const float4 &q) { return make_float4(p.x * q.x, p.y * q.y, p.z * q.z, p.w * q.w); }
__device__ __forceinline__ float4 ln_add(const float4 &p, const float4 &q) { return make_float4(p.x + q.x, p.y + q.y, p.z + q.z, p.w + q.w); }
__device__ __forceinline__ float4 ln_zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
// four consecutive floats of a vector nobody promised to align (a, b)
__device__ __forceinline__ float4 ln_load4(const float *p) { return make_float4(p[0], p[1], p[2], p[3]); }

// A lane's groups of four columns: group lane + 64 j, j < NV, live where it is below nvec = d / 4.
template <int NV>
__global__ __launch_bounds__(kLnThreads) void ln_forward_kernel(int rows, int d, const float *__restrict__ x,
                                                                const float *__restrict__ delta,
                                                                const float *__restrict__ a, const float *__restrict__ b,
                                                                float eps, float *__restrict__ sum, float *__restrict__ y,
                                                                float *__restrict__ stats) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nvec = d >> 2;
  float4 av[NV], bv[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int g = lane + 64 * j;
    av[j] = g < nvec ? ln_load4(a + 4 * g) : ln_zero();
    bv[j] = g < nvec ? ln_load4(b + 4 * g) : ln_zero();
  }
  const float fd = (float)d, fd1 = (float)(d - 1);
  for (int row = blockIdx.x * kLnWaves + wave; row < rows; row += gridDim.x * kLnWaves) {
    const size_t base = (size_t)row * d;
    float4 z[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int g = lane + 64 * j;
      z[j] = g < nvec ? *reinterpret_cast<const float4 *>(x + base + 4 * g) : ln_zero();
    }
    if (delta) {
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        const int g = lane + 64 * j;
        if (g < nvec) z[j] = ln_add(z[j], *reinterpret_cast<const float4 *>(delta + base + 4 * g));
      }
    }
    if (sum) {
#pragma unroll
      for (int j = 0; j < NV; ++j) {
        const int g = lane + 64 * j;
        if (g < nvec) *reinterpret_cast<float4 *>(sum + base + 4 * g) = z[j];
      }
    }
    float s = ln_lane_sum(z[0]);
#pragma unroll
    for (int j = 1; j < NV; ++j) s += ln_lane_sum(z[j]);
    const float mean = wave_sum(s) / fd;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      z[j] = lane + 64 * j < nvec ? ln_sub(z[j], mean) : ln_zero();      // a dead group must not reach the variance
      const float t = ln_lane_sum(ln_mul(z[j], z[j]));
      q = j == 0 ? t : q + t;
    }
    const float sd = __builtin_sqrtf(wave_sum(q) / fd1);
    const float u = 1.f / (sd + eps);
    if (stats && lane == 0) {
      stats[2 * (size_t)row] = mean;
      stats[2 * (size_t)row + 1] = sd;
    }
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int g = lane + 64 * j;
      if (g < nvec) {
        const float4 o = make_float4((av[j].x * z[j].x) * u + bv[j].x, (av[j].y * z[j].y) * u + bv[j].y,
                                     (av[j].z * z[j].z) * u + bv[j].z, (av[j].w * z[j].w) * u + bv[j].w);
        *reinterpret_cast<float4 *>(y + base + 4 * g) = o;
      }
    }
  }
}

// slabs: one [2][d] per workgroup ({ga, gb} summed over the workgroup's rows), or NULL (no ga / gb wanted).
// Dynamic LDS: kLnWaves * 2 * d floats when slabs is given.
template <int NV>
__global__ __launch_bounds__(kLnThreads, 4) void ln_backward_kernel(int rows, int d, const float *__restrict__ zin,
                                                                 const float *__restrict__ a,
                                                                 const float *__restrict__ gy,
                                                                 const float *__restrict__ gres,
                                                                 const float *__restrict__ stats, float eps,
                                                                 float *__restrict__ gz, float *__restrict__ slabs) {
  extern __shared__ __attribute__((aligned(16))) float ln_part[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nvec = d >> 2;
  // Up to three groups a lane everything a row needs is held or asked for at its start, and the column sums grow in
  // registers.  With four, 4 waves per SIMD leave 128 registers: `a` is read again in every row (it stays in the cache), the
  // residual stream's gradient after the sums, and the column sums grow in the wave's own slice of LDS.
  constexpr bool kHold = NV <= 3;
  float4 ah[kHold ? NV : 1], pa[kHold ? NV : 1], pb[kHold ? NV : 1];
  float *mine = ln_part + (size_t)(wave * 2) * d;              // [{ga, gb}][d], touched only when slabs is given
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int g = lane + 64 * j;
    if (kHold) {
      ah[j] = g < nvec ? ln_load4(a + 4 * g) : ln_zero();
      pa[j] = pb[j] = ln_zero();
    } else if (slabs && g < nvec) {
      *reinterpret_cast<float4 *>(mine + 4 * g) = ln_zero();
      *reinterpret_cast<float4 *>(mine + d + 4 * g) = ln_zero();
    }
  }
  const float fd = (float)d, fd1 = (float)(d - 1);
  for (int row = blockIdx.x * kLnWaves + wave; row < rows; row += gridDim.x * kLnWaves) {
    float4 av[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j)
      av[j] = kHold ? ah[j] : lane + 64 * j < nvec ? ln_load4(a + 4 * (lane + 64 * j)) : ln_zero();
    const size_t base = (size_t)row * d;
    const float mean = stats[2 * (size_t)row], sd = stats[2 * (size_t)row + 1];
    constexpr bool kEarly = kHold;
    float4 c[NV], g4[NV], gr[kEarly ? NV : 1];
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int g = lane + 64 * j;
      c[j] = g < nvec ? *reinterpret_cast<const float4 *>(zin + base + 4 * g) : ln_zero();
      g4[j] = g < nvec ? *reinterpret_cast<const float4 *>(gy + base + 4 * g) : ln_zero();
      if (kEarly) gr[j] = (gres && g < nvec) ? *reinterpret_cast<const float4 *>(gres + base + 4 * g) : ln_zero();
    }
    // The centred values, each to a relative rounding: z - mean is exact in double, and so (to 2^-53) is the sum that tells
    // how far the float32 mean is off the row's mean; with that taken out a value NEAR the mean keeps its digits.  (In float32
    // alone c carries the mean's rounding, an absolute u * mean|z|: nothing next to y or gz, but all there is of a column sum
    // ga over a few rows whose c is small.)
    double cs = 0.0;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      if (lane + 64 * j < nvec)
        cs += (((double)c[j].x - (double)mean) + ((double)c[j].y - (double)mean)) +
              (((double)c[j].z - (double)mean) + ((double)c[j].w - (double)mean));
    }
    const double off = (double)mean + wave_sum(cs) / (double)d;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      c[j] = lane + 64 * j < nvec ? make_float4((float)((double)c[j].x - off), (float)((double)c[j].y - off),
                                                (float)((double)c[j].z - off), (float)((double)c[j].w - off))
                                  : ln_zero();
      const float4 gh = ln_mul(g4[j], av[j]);
      const float t1 = ln_lane_sum(gh), t2 = ln_lane_sum(ln_mul(gh, c[j]));
      s1 = j == 0 ? t1 : s1 + t1;
      s2 = j == 0 ? t2 : s2 + t2;
    }
    const float u = 1.f / (sd + eps);
    const float mgh = wave_sum(s1) / fd;
    const float dot = wave_sum(s2);
    const float coef = sd == 0.f ? 0.f : ((dot * u) * u) / (fd1 * sd);      // a NaN std is not 0: the row comes out NaN
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int g = lane + 64 * j;
      if (g < nvec) {
        const float4 gh = ln_mul(g4[j], av[j]);
        float4 o = make_float4(u * (gh.x - mgh) - c[j].x * coef, u * (gh.y - mgh) - c[j].y * coef,
                               u * (gh.z - mgh) - c[j].z * coef, u * (gh.w - mgh) - c[j].w * coef);
        if (gres) o = ln_add(o, kEarly ? gr[j] : *reinterpret_cast<const float4 *>(gres + base + 4 * g));
        *reinterpret_cast<float4 *>(gz + base + 4 * g) = o;
      }
      if (slabs) {
        const float4 ta = make_float4((g4[j].x * c[j].x) * u, (g4[j].y * c[j].y) * u, (g4[j].z * c[j].z) * u,
                                      (g4[j].w * c[j].w) * u);
        if (kHold) {
          pa[j] = ln_add(pa[j], ta);
          pb[j] = ln_add(pb[j], g4[j]);
        } else if (g < nvec) {                                   // a lane's own words: no other lane reads them before the barrier
          float4 *qa = reinterpret_cast<float4 *>(mine + 4 * g), *qb = reinterpret_cast<float4 *>(mine + d + 4 * g);
          *qa = ln_add(*qa, ta);
          *qb = ln_add(*qb, g4[j]);
        }
      }
    }
  }
  if (!slabs) return;
  // the four waves' column sums, added in wave order: ln_part[wave][{ga, gb}][d]
  if (kHold) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int g = lane + 64 * j;
      if (g < nvec) {
        *reinterpret_cast<float4 *>(mine + 4 * g) = pa[j];
        *reinterpret_cast<float4 *>(mine + d + 4 * g) = pb[j];
      }
    }
  }
  __syncthreads();
  float *slab = slabs + (size_t)blockIdx.x * 2 * d;
  for (int i = threadIdx.x; i < 2 * d; i += kLnThreads) {
    float v = ln_part[i];
#pragma unroll
    for (int w = 1; w < kLnWaves; ++w) v += ln_part[(size_t)w * 2 * d + i];
    slab[i] = v;
  }
}

// {ga, gb}[i] = sum over the nslab slabs of slab[s][i], i < 2 d (ga takes the first d sums, gb the rest; either may be
// NULL).  A workgroup of 64 columns x kLnSumParts runs of slabs: thread (part, col) adds its run in ascending order, the
// parts are then added in order.
__global__ __launch_bounds__(64 * kLnSumParts) void ln_slab_sum_kernel(int nslab, int d, const float *__restrict__ slabs,
                                                                       float *__restrict__ ga, float *__restrict__ gb) {
  __shared__ float part[kLnSumParts][64];
  const int col = threadIdx.x & 63, p = threadIdx.x >> 6, len = 2 * d;
  const int i = blockIdx.x * 64 + col;
  const int run = (nslab + kLnSumParts - 1) / kLnSumParts;
  const int s0 = p * run, s1 = min(nslab, s0 + run);
  float v = 0.f;
  if (i < len) {
#pragma unroll 8
    for (int s = s0; s < s1; ++s) v += slabs[(size_t)s * len + i];
  }
  part[p][col] = v;
  __syncthreads();
  if (p == 0 && i < len) {
    float t = part[0][col];
#pragma unroll
    for (int k = 1; k < kLnSumParts; ++k) t += part[k][col];
    if (i < d) {
      if (ga) ga[i] = t;
    } else if (gb) {
      gb[i - d] = t;
    }
  }
}

static bool ln_shape_ok(int rows, int d) {
  return rows >= 0 && d >= 4 && d <= kLnMaxD && (d & 3) == 0 && (long long)rows * d < 2147483648LL;
}

}  // namespace mvp

using namespace mvp;

// KERNEL<NV> for NV = ceil(d / 256) float4 a lane; `grid`, `block` and `st` are the caller's.
#define MVP_LN_LAUNCH(KERNEL, LDS, ...)                                                    \
  switch ((d + 255) / 256) {                                                               \
    case 1: hipLaunchKernelGGL(KERNEL<1>, grid, block, LDS, st, __VA_ARGS__); break;       \
    case 2: hipLaunchKernelGGL(KERNEL<2>, grid, block, LDS, st, __VA_ARGS__); break;       \
    case 3: hipLaunchKernelGGL(KERNEL<3>, grid, block, LDS, st, __VA_ARGS__); break;       \
    default: hipLaunchKernelGGL(KERNEL<4>, grid, block, LDS, st, __VA_ARGS__); break;      \
  }

extern "C" int mvp_ref_layernorm(int rows, int d, const float *x, const float *delta, const float *a, const float *b,
                                 float eps, float *sum, float *y, float *stats, void *stream) {
  if (!ln_shape_ok(rows, d)) return MVP_EBADSHAPE;
  if (bad_eps(eps)) return MVP_EBADARG;
  if (misaligned(x) || misaligned(delta) || misaligned(sum) || misaligned(y)) return MVP_EBADARG;
  if (rows == 0) return MVP_OK;
  if (!x || !a || !b || !y || (delta && !sum)) return MVP_EBADARG;
  const dim3 grid((unsigned)ln_grid(rows)), block(kLnThreads);
  hipStream_t st = as_stream(stream);
  MVP_LN_LAUNCH(ln_forward_kernel, 0, rows, d, x, delta, a, b, eps, sum, y, stats);
  return check_launch("mvp_ref_layernorm");
}

extern "C" long long mvp_ref_layernorm_backward_scratch_bytes(int rows, int d) {
  if (!ln_shape_ok(rows, d) || rows == 0) return 0;
  return (long long)ln_grid(rows) * 2 * d * (long long)sizeof(float);
}

extern "C" int mvp_ref_layernorm_backward(int rows, int d, const float *z, const float *a, const float *gy,
                                          const float *gres, const float *stats, float eps, float *gz, float *ga,
                                          float *gb, void *scratch, long long scratch_bytes, void *stream) {
  if (!ln_shape_ok(rows, d)) return MVP_EBADSHAPE;
  if (bad_eps(eps)) return MVP_EBADARG;
  if (misaligned(z) || misaligned(gy) || misaligned(gres) || misaligned(gz)) return MVP_EBADARG;
  if (rows == 0) return MVP_OK;      // nothing to add: ga / gb of an empty batch are the caller's zeros
  if (!z || !a || !gy || !stats || !gz) return MVP_EBADARG;
  const bool cols = ga || gb;
  if (cols && scratch_short(scratch, scratch_bytes, mvp_ref_layernorm_backward_scratch_bytes(rows, d))) return MVP_EBADARG;
  const int nb = ln_grid(rows);
  const dim3 grid((unsigned)nb), block(kLnThreads);
  const size_t lds = cols ? (size_t)kLnWaves * 2 * d * sizeof(float) : 0;
  float *slabs = cols ? static_cast<float *>(scratch) : nullptr;
  hipStream_t st = as_stream(stream);
  MVP_LN_LAUNCH(ln_backward_kernel, lds, rows, d, z, a, gy, gres, stats, eps, gz, slabs);
  if (cols) {
    const int rc = check_launch("mvp_ref_layernorm_backward");
    if (rc != MVP_OK) return rc;
    hipLaunchKernelGGL(ln_slab_sum_kernel, dim3((unsigned)((2 * d + 63) / 64)), dim3(64 * kLnSumParts), 0, st, nb, d,
                       slabs, ga, gb);
  }
  return check_launch("mvp_ref_layernorm_backward");
}
