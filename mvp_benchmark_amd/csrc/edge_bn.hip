// DGCNN's BatchNorm2d -> ReLU -> max over the k neighbours as DCP trains it (registration/models/dcp.py: DGCNN; reference
// dcp.py:286-318), forward and backward, on z (b, c, k, n): neighbours on the slow axis, n contiguous, M = b k n per channel.
//   batch statistics:   mean_c = sum z / M,  var_c = sum (z - mean_c)^2 / M  (biased, centred),  invstd_c = 1 / sqrt(var_c + eps)
//   running statistics: stats = {running_mean_c, 1 / sqrt(running_var_c + eps)}, filled by the caller
//   y = fmaf(z - mean_c, gamma_c * invstd_c, beta_c)  (ebn_y: the ONE expression forward and backward evaluate)
//   r = relu(y),  pooled = max_j r,  arg = the lowest j attaining it
//   g_y = (g_r + [j == arg] g_pool) where y > 0;  gbeta = sum g_y,  ggamma = sum g_y xhat,  xhat = (z - mean_c) invstd_c
//   gz = gamma_c invstd_c (g_y - gbeta / M - xhat ggamma / M)   (running statistics: gamma_c invstd_c g_y)
// The composed route runs this as conv -> BatchNorm (statistics + map) -> ReLU -> max, keeps the BatchNorm's and the ReLU's
// outputs for autograd, and on the way back scatters the max's gradient, adds it, masks it and runs BatchNorm's two backward
// passes.  Here: z is read for the statistics, read and (r wanted) written once for the map; backward reads z and g_r
// twice and writes gz once.
//
// Work split: one workgroup per (b, c) slab -- k n contiguous floats, 80 KB at cfg 5 -- in every kernel: 512 lanes for the
// statistics (their double arithmetic is the one part that is not free: at 256 lanes and 20 float4 a lane two workgroups a
// CU alternated between loading and adding, 2.7-3.2 TB/s), 256 lanes elsewhere.
// The statistics are a pass of their own because y needs the channel's mean and variance over ALL b slabs before its first
// element can be formed; a slab's {mean, M2} is exact to double (per-lane double sums, wave_sum's fixed tree, the waves
// in order; M2 from values centred on the slab's own mean, the slab held in registers between the two sweeps up to
// kEbHold float4 a lane, re-read above), and ebn_stats_merge_kernel folds the b slabs of a channel in ascending b with
// Chan's update.  The backward sums go the same way.  No atomics, nothing passes between workgroups inside a launch: the
// same bits on every run.  double costs nothing here: the kernels wait for memory.
// In the map and the backward sweeps a lane owns groups of four columns (float4) and walks k, kEbAhead loads in flight.
// Non-finite values and the dead channel: include/mvpops.h.  The entry points' guards: common.h.
#include "common.h"
#include "wave.h"

namespace mvp {

constexpr int kEbThreads = 256;
constexpr int kEbWaves = kEbThreads / kWave;
constexpr int kEbStatThreads = 512;      // the statistics kernel: eight waves share a slab's double arithmetic
constexpr int kEbStatWaves = kEbStatThreads / kWave;
constexpr int kEbHold = 10;       // float4 a lane keeps between the two sweeps of a slab: 512 * 10 * 4 = 20480 floats = cfg 5's k n
constexpr int kEbAhead = 4;       // neighbours (float4 loads per operand) a lane has in flight
constexpr int kEbMaxK = 64;

// The map, shared by every kernel below: the backward pass's mask y > 0 has the forward's bits.
__device__ __forceinline__ float ebn_y(float z, float mean, float scale, float beta) { return __builtin_fmaf(z - mean, scale, beta); }
__device__ __forceinline__ float ebn_relu(float y) { return y <= 0.f ? 0.f : y; }      // a NaN is not <= 0: it stays
__device__ __forceinline__ float ebn_xhat(float z, float mean, float invstd) { return (z - mean) * invstd; }
__device__ __forceinline__ float4 ebn_zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// The sum over the workgroup of one double per lane, in every lane: wave_sum's tree, then the waves in order.  Holds two
// barriers: every thread calls it.
template <int WAVES>
__device__ __forceinline__ double ebn_block_sum(double v, double *red) {
  v = wave_sum(v);
  __syncthreads();                                  // the previous sum has been read
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = red[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) t += red[w];
  return t;
}

__device__ __forceinline__ double ebn_sum4(const float4 &v) {
  return ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
}
__device__ __forceinline__ double ebn_sq4(const float4 &v, double m) {
  const double a = (double)v.x - m, b = (double)v.y - m, c = (double)v.z - m, d = (double)v.w - m;
  return (a * a + b * b) + (c * c + d * d);
}

// part[slab] = {mean, M2} of the slab's 4 nvec floats.  HOLD: nvec <= kEbStatThreads * kEbHold.
template <bool HOLD>
__global__ __launch_bounds__(kEbStatThreads) void ebn_slab_stats_kernel(int nvec, const float *__restrict__ z,
                                                                    double *__restrict__ part) {
  __shared__ double red[kEbStatWaves];
  const float4 *p = reinterpret_cast<const float4 *>(z + (size_t)blockIdx.x * 4 * (size_t)nvec);
  const int t = threadIdx.x;
  float4 held[HOLD ? kEbHold : 1];
  double s = 0.0;
  if constexpr (HOLD) {
#pragma unroll
    for (int i = 0; i < kEbHold; ++i) {
      const int g = t + kEbStatThreads * i;
      held[i] = g < nvec ? p[g] : ebn_zero4();
    }
#pragma unroll
    for (int i = 0; i < kEbHold; ++i) s += ebn_sum4(held[i]);          // a dead group adds 0
  } else {
    for (int g0 = t; g0 < nvec; g0 += kEbStatThreads * kEbAhead) {
      float4 v[kEbAhead];
#pragma unroll
      for (int u = 0; u < kEbAhead; ++u) v[u] = g0 + kEbStatThreads * u < nvec ? p[g0 + kEbStatThreads * u] : ebn_zero4();
#pragma unroll
      for (int u = 0; u < kEbAhead; ++u) s += ebn_sum4(v[u]);
    }
  }
  const double mean = ebn_block_sum<kEbStatWaves>(s, red) / (4.0 * (double)nvec);
  double q = 0.0;
  if constexpr (HOLD) {
#pragma unroll
    for (int i = 0; i < kEbHold; ++i)
      if (t + kEbStatThreads * i < nvec) q += ebn_sq4(held[i], mean);
  } else {
    for (int g0 = t; g0 < nvec; g0 += kEbStatThreads * kEbAhead) {
      float4 v[kEbAhead];
#pragma unroll
      for (int u = 0; u < kEbAhead; ++u) v[u] = g0 + kEbStatThreads * u < nvec ? p[g0 + kEbStatThreads * u] : ebn_zero4();
#pragma unroll
      for (int u = 0; u < kEbAhead; ++u)
        if (g0 + kEbStatThreads * u < nvec) q += ebn_sq4(v[u], mean);
    }
  }
  const double m2 = ebn_block_sum<kEbStatWaves>(q, red);
  if (t == 0) {
    part[2 * (size_t)blockIdx.x] = mean;
    part[2 * (size_t)blockIdx.x + 1] = m2;
  }
}

// One lane per channel: the b slabs of len values each, in ascending b (Chan et al.: the mean of i + 1 slabs from the mean
// of i and the next one, M2 with the between-slab term).  A non-finite slab makes M2, hence var, NaN; the mean follows it.
__global__ __launch_bounds__(kWave) void ebn_stats_merge_kernel(int b, int c, double len, float eps,
                                                                const double *__restrict__ part,
                                                                float *__restrict__ stats, float *__restrict__ var) {
  const int ch = blockIdx.x * kWave + threadIdx.x;
  if (ch >= c) return;
  double mean = part[2 * (size_t)ch], m2 = part[2 * (size_t)ch + 1];
  for (int i = 1; i < b; ++i) {
    const double *p = part + 2 * ((size_t)i * c + ch);
    const double d = p[0] - mean;
    mean += d / (double)(i + 1);
    m2 += p[1] + (d * d) * (len * ((double)i / (double)(i + 1)));
  }
  const double v = m2 / (len * (double)b);
  if (v != v) mean = v;
  stats[2 * (size_t)ch] = (float)mean;
  stats[2 * (size_t)ch + 1] = (float)(1.0 / __builtin_sqrt(v + (double)eps));
  var[ch] = (float)v;
}

// One component of a column group: the running maximum and its neighbour.  Replaced only by a value that is not <= the
// maximum (greater, or the first NaN), and never once the maximum is a NaN: the lowest j wins a tie.
__device__ __forceinline__ void ebn_take(float r, int j, float &best, unsigned &at) {
  if (!(r <= best) && best == best) {
    best = r;
    at = (unsigned)j;
  }
}

template <bool WRITE_R>
__global__ __launch_bounds__(kEbThreads) void ebn_relu_max_kernel(int c, int k, int n, const float *__restrict__ z,
                                                                  const float *__restrict__ stats,
                                                                  const float *__restrict__ gamma,
                                                                  const float *__restrict__ beta, float *__restrict__ r,
                                                                  float *__restrict__ pooled,
                                                                  unsigned char *__restrict__ arg) {
  const int ch = blockIdx.x % c, nv = n >> 2;
  const float mean = stats[2 * ch], scale = gamma[ch] * stats[2 * ch + 1], bt = beta[ch];
  const size_t slab = (size_t)blockIdx.x * ((size_t)k * n);
  const float4 *zp = reinterpret_cast<const float4 *>(z + slab);
  float4 *rp = WRITE_R ? reinterpret_cast<float4 *>(r + slab) : nullptr;
  float4 *pp = reinterpret_cast<float4 *>(pooled + (size_t)blockIdx.x * n);
  unsigned *ap = reinterpret_cast<unsigned *>(arg + (size_t)blockIdx.x * n);
  for (int g = threadIdx.x; g < nv; g += kEbThreads) {
    float4 best = ebn_zero4();
    unsigned a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    for (int j0 = 0; j0 < k; j0 += kEbAhead) {
      float4 v[kEbAhead];
#pragma unroll
      for (int u = 0; u < kEbAhead; ++u)
        if (j0 + u < k) v[u] = zp[(size_t)(j0 + u) * nv + g];
#pragma unroll
      for (int u = 0; u < kEbAhead; ++u) {
        const int j = j0 + u;
        if (j < k) {
          const float4 y = make_float4(ebn_relu(ebn_y(v[u].x, mean, scale, bt)), ebn_relu(ebn_y(v[u].y, mean, scale, bt)),
                                       ebn_relu(ebn_y(v[u].z, mean, scale, bt)), ebn_relu(ebn_y(v[u].w, mean, scale, bt)));
          if (WRITE_R) rp[(size_t)j * nv + g] = y;
          if (j == 0) {
            best = y;
          } else {
            ebn_take(y.x, j, best.x, a0);
            ebn_take(y.y, j, best.y, a1);
            ebn_take(y.z, j, best.z, a2);
            ebn_take(y.w, j, best.w, a3);
          }
        }
      }
    }
    pp[g] = best;
    ap[g] = a0 | (a1 << 8) | (a2 << 16) | (a3 << 24);
  }
}

// g_y of four columns at neighbour j: (g_r + [j == arg] g_pool) where y > 0, else 0 -- a selection, never a product, so a
// masked element is exactly 0.  at: the group's four arg bytes.
__device__ __forceinline__ float ebn_gy1(float z, float gr, float gp, bool hit, float mean, float scale, float bt) {
  const float g = hit ? gr + gp : gr;
  return ebn_y(z, mean, scale, bt) > 0.f ? g : 0.f;
}
__device__ __forceinline__ float4 ebn_gy4(const float4 &z, const float4 &gr, const float4 &gp, unsigned at, int j, float mean,
                                          float scale, float bt) {
  const unsigned uj = (unsigned)j;
  return make_float4(ebn_gy1(z.x, gr.x, gp.x, (at & 255u) == uj, mean, scale, bt),
                     ebn_gy1(z.y, gr.y, gp.y, ((at >> 8) & 255u) == uj, mean, scale, bt),
                     ebn_gy1(z.z, gr.z, gp.z, ((at >> 16) & 255u) == uj, mean, scale, bt),
                     ebn_gy1(z.w, gr.w, gp.w, (at >> 24) == uj, mean, scale, bt));
}

// Pass 1: part[slab] = {sum g_y, sum g_y xhat} of the slab.
__global__ __launch_bounds__(kEbThreads) void ebn_backward_sums_kernel(int c, int k, int n, const float *__restrict__ z,
                                                                       const float *__restrict__ stats,
                                                                       const float *__restrict__ gamma,
                                                                       const float *__restrict__ beta,
                                                                       const unsigned char *__restrict__ arg,
                                                                       const float *__restrict__ g_r,
                                                                       const float *__restrict__ g_pool,
                                                                       double *__restrict__ part) {
  __shared__ double red[kEbWaves];
  const int ch = blockIdx.x % c, nv = n >> 2;
  const float mean = stats[2 * ch], invstd = stats[2 * ch + 1], scale = gamma[ch] * invstd, bt = beta[ch];
  const size_t slab = (size_t)blockIdx.x * ((size_t)k * n);
  const float4 *zp = reinterpret_cast<const float4 *>(z + slab);
  const float4 *gp = g_r ? reinterpret_cast<const float4 *>(g_r + slab) : nullptr;
  const float4 *pp = g_pool ? reinterpret_cast<const float4 *>(g_pool + (size_t)blockIdx.x * n) : nullptr;
  const unsigned *ap = reinterpret_cast<const unsigned *>(arg + (size_t)blockIdx.x * n);
  double s1 = 0.0, s2 = 0.0;
  for (int g = threadIdx.x; g < nv; g += kEbThreads) {
    const float4 pool = pp ? pp[g] : ebn_zero4();
    const unsigned at = pp ? ap[g] : 0xFFFFFFFFu;              // no pooled gradient: no neighbour is hit (j <= 63)
    for (int j0 = 0; j0 < k; j0 += kEbAhead) {
      float4 v[kEbAhead], w[kEbAhead];
#pragma unroll
      for (int u = 0; u < kEbAhead; ++u) {
        if (j0 + u < k) {
          v[u] = zp[(size_t)(j0 + u) * nv + g];
          w[u] = gp ? gp[(size_t)(j0 + u) * nv + g] : ebn_zero4();
        }
      }
#pragma unroll
      for (int u = 0; u < kEbAhead; ++u) {
        if (j0 + u < k) {
          const float4 gy = ebn_gy4(v[u], w[u], pool, at, j0 + u, mean, scale, bt);
          s1 += ebn_sum4(gy);
          s2 += ((double)(gy.x * ebn_xhat(v[u].x, mean, invstd)) + (double)(gy.y * ebn_xhat(v[u].y, mean, invstd))) +
                ((double)(gy.z * ebn_xhat(v[u].z, mean, invstd)) + (double)(gy.w * ebn_xhat(v[u].w, mean, invstd)));
        }
      }
    }
  }
  s1 = ebn_block_sum<kEbWaves>(s1, red);
  s2 = ebn_block_sum<kEbWaves>(s2, red);
  if (threadIdx.x == 0) {
    part[2 * (size_t)blockIdx.x] = s1;
    part[2 * (size_t)blockIdx.x + 1] = s2;
  }
}

// One lane per channel: the b partial sums in ascending b -> gbeta, ggamma (each may be NULL) and coef[ch] = the two
// sums over M, what pass 2 takes off g_y.
__global__ __launch_bounds__(kWave) void ebn_backward_merge_kernel(int b, int c, double m, const double *__restrict__ part,
                                                                   float *__restrict__ ggamma, float *__restrict__ gbeta,
                                                                   float *__restrict__ coef) {
  const int ch = blockIdx.x * kWave + threadIdx.x;
  if (ch >= c) return;
  double s1 = 0.0, s2 = 0.0;
  for (int i = 0; i < b; ++i) {
    const double *p = part + 2 * ((size_t)i * c + ch);
    s1 += p[0];
    s2 += p[1];
  }
  if (gbeta) gbeta[ch] = (float)s1;
  if (ggamma) ggamma[ch] = (float)s2;
  coef[2 * (size_t)ch] = (float)(s1 / m);
  coef[2 * (size_t)ch + 1] = (float)(s2 / m);
}

// Pass 2: gz.  BATCH: the two channel sums over M come off g_y (coef); otherwise the map is elementwise.
template <bool BATCH>
__global__ __launch_bounds__(kEbThreads) void ebn_backward_gz_kernel(int c, int k, int n, const float *__restrict__ z,
                                                                     const float *__restrict__ stats,
                                                                     const float *__restrict__ gamma,
                                                                     const float *__restrict__ beta,
                                                                     const unsigned char *__restrict__ arg,
                                                                     const float *__restrict__ g_r,
                                                                     const float *__restrict__ g_pool,
                                                                     const float *__restrict__ coef,
                                                                     float *__restrict__ gz) {
  const int ch = blockIdx.x % c, nv = n >> 2;
  const float mean = stats[2 * ch], invstd = stats[2 * ch + 1], scale = gamma[ch] * invstd, bt = beta[ch];
  const float c1 = BATCH ? coef[2 * ch] : 0.f, c2 = BATCH ? coef[2 * ch + 1] : 0.f;
  const size_t slab = (size_t)blockIdx.x * ((size_t)k * n);
  const float4 *zp = reinterpret_cast<const float4 *>(z + slab);
  const float4 *gp = g_r ? reinterpret_cast<const float4 *>(g_r + slab) : nullptr;
  const float4 *pp = g_pool ? reinterpret_cast<const float4 *>(g_pool + (size_t)blockIdx.x * n) : nullptr;
  const unsigned *ap = reinterpret_cast<const unsigned *>(arg + (size_t)blockIdx.x * n);
  float4 *op = reinterpret_cast<float4 *>(gz + slab);
  for (int g = threadIdx.x; g < nv; g += kEbThreads) {
    const float4 pool = pp ? pp[g] : ebn_zero4();
    const unsigned at = pp ? ap[g] : 0xFFFFFFFFu;
    for (int j0 = 0; j0 < k; j0 += kEbAhead) {
      float4 v[kEbAhead], w[kEbAhead];
#pragma unroll
      for (int u = 0; u < kEbAhead; ++u) {
        if (j0 + u < k) {
          v[u] = zp[(size_t)(j0 + u) * nv + g];
          w[u] = gp ? gp[(size_t)(j0 + u) * nv + g] : ebn_zero4();
        }
      }
#pragma unroll
      for (int u = 0; u < kEbAhead; ++u) {
        if (j0 + u < k) {
          const float4 gy = ebn_gy4(v[u], w[u], pool, at, j0 + u, mean, scale, bt);
          float4 o;
          if (BATCH) {
            o = make_float4(scale * ((gy.x - c1) - ebn_xhat(v[u].x, mean, invstd) * c2),
                            scale * ((gy.y - c1) - ebn_xhat(v[u].y, mean, invstd) * c2),
                            scale * ((gy.z - c1) - ebn_xhat(v[u].z, mean, invstd) * c2),
                            scale * ((gy.w - c1) - ebn_xhat(v[u].w, mean, invstd) * c2));
          } else {
            o = make_float4(scale * gy.x, scale * gy.y, scale * gy.z, scale * gy.w);
          }
          op[(size_t)(j0 + u) * nv + g] = o;
        }
      }
    }
  }
}

static bool ebn_shape_ok(int b, int c, int k, int n) {
  return b >= 1 && c >= 1 && k >= 1 && k <= kEbMaxK && n >= 4 && (n & 3) == 0 && (long long)k * n < 2147483648LL &&
         (long long)b * c < 2147483648LL;
}
// {partials: [b c][2] double} {coef: [c][2] float}, the second part on a 16-byte address
static long long ebn_part_bytes(int b, int c) { return (long long)b * c * 2 * (long long)sizeof(double); }

}  // namespace mvp

using namespace mvp;

extern "C" long long mvp_edge_bn_scratch_bytes(int b, int c) {
  if (b < 1 || c < 1 || (long long)b * c >= 2147483648LL) return 0;
  return ebn_part_bytes(b, c) + (((long long)c * 2 * (long long)sizeof(float) + 15) & ~15LL);
}

extern "C" int mvp_edge_bn_stats(int b, int c, int k, int n, const float *z, float eps, float *stats, float *var,
                                 void *scratch, long long scratch_bytes, void *stream) {
  if (!ebn_shape_ok(b, c, k, n)) return MVP_EBADSHAPE;
  if (bad_eps(eps)) return MVP_EBADARG;
  if (misaligned(z)) return MVP_EBADARG;
  if (!z || !stats || !var) return MVP_EBADARG;
  if (scratch_short(scratch, scratch_bytes, mvp_edge_bn_scratch_bytes(b, c))) return MVP_EBADARG;
  hipStream_t st = as_stream(stream);
  double *part = static_cast<double *>(scratch);
  const int nvec = (int)(((long long)k * n) >> 2);
  const dim3 grid((unsigned)(b * c)), block(kEbStatThreads);
  if (nvec <= kEbStatThreads * kEbHold)
    hipLaunchKernelGGL(ebn_slab_stats_kernel<true>, grid, block, 0, st, nvec, z, part);
  else
    hipLaunchKernelGGL(ebn_slab_stats_kernel<false>, grid, block, 0, st, nvec, z, part);
  const int rc = check_launch("mvp_edge_bn_stats");
  if (rc != MVP_OK) return rc;
  hipLaunchKernelGGL(ebn_stats_merge_kernel, dim3((unsigned)((c + kWave - 1) / kWave)), dim3(kWave), 0, st, b, c,
                     (double)k * (double)n, eps, part, stats, var);
  return check_launch("mvp_edge_bn_stats");
}

extern "C" int mvp_edge_bn_relu_max(int b, int c, int k, int n, const float *z, const float *stats, const float *gamma,
                                    const float *beta, float *r, float *pooled, unsigned char *arg, void *stream) {
  if (!ebn_shape_ok(b, c, k, n)) return MVP_EBADSHAPE;
  if (misaligned(z) || misaligned(r) || misaligned(pooled) || misaligned(arg, 3)) return MVP_EBADARG;
  if (!z || !stats || !gamma || !beta || !pooled || !arg) return MVP_EBADARG;
  const dim3 grid((unsigned)(b * c)), block(kEbThreads);
  hipStream_t st = as_stream(stream);
  if (r)
    hipLaunchKernelGGL(ebn_relu_max_kernel<true>, grid, block, 0, st, c, k, n, z, stats, gamma, beta, r, pooled, arg);
  else
    hipLaunchKernelGGL(ebn_relu_max_kernel<false>, grid, block, 0, st, c, k, n, z, stats, gamma, beta, r, pooled, arg);
  return check_launch("mvp_edge_bn_relu_max");
}

extern "C" int mvp_edge_bn_relu_max_backward(int b, int c, int k, int n, int batch_stats, const float *z, const float *stats,
                                             const float *gamma, const float *beta, const unsigned char *arg,
                                             const float *g_r, const float *g_pool, float *gz, float *ggamma, float *gbeta,
                                             void *scratch, long long scratch_bytes, void *stream) {
  if (!ebn_shape_ok(b, c, k, n)) return MVP_EBADSHAPE;
  if (misaligned(z) || misaligned(g_r) || misaligned(g_pool) || misaligned(gz) || misaligned(arg, 3)) return MVP_EBADARG;
  if (!g_r && !g_pool) return MVP_EBADARG;
  if (!z || !stats || !gamma || !beta || !gz || (g_pool && !arg)) return MVP_EBADARG;
  const bool sums = batch_stats || ggamma || gbeta;
  if (sums && scratch_short(scratch, scratch_bytes, mvp_edge_bn_scratch_bytes(b, c))) return MVP_EBADARG;
  const dim3 grid((unsigned)(b * c)), block(kEbThreads);
  hipStream_t st = as_stream(stream);
  double *part = static_cast<double *>(scratch);
  float *coef = sums ? reinterpret_cast<float *>(static_cast<char *>(scratch) + ebn_part_bytes(b, c)) : nullptr;
  if (sums) {
    hipLaunchKernelGGL(ebn_backward_sums_kernel, grid, block, 0, st, c, k, n, z, stats, gamma, beta, arg, g_r, g_pool, part);
    int rc = check_launch("mvp_edge_bn_relu_max_backward");
    if (rc != MVP_OK) return rc;
    hipLaunchKernelGGL(ebn_backward_merge_kernel, dim3((unsigned)((c + kWave - 1) / kWave)), dim3(kWave), 0, st, b, c,
                       (double)b * (double)k * (double)n, part, ggamma, gbeta, coef);
    rc = check_launch("mvp_edge_bn_relu_max_backward");
    if (rc != MVP_OK) return rc;
  }
  if (batch_stats)
    hipLaunchKernelGGL(ebn_backward_gz_kernel<true>, grid, block, 0, st, c, k, n, z, stats, gamma, beta, arg, g_r, g_pool,
                       coef, gz);
  else
    hipLaunchKernelGGL(ebn_backward_gz_kernel<false>, grid, block, 0, st, c, k, n, z, stats, gamma, beta, arg, g_r, g_pool,
                       coef, gz);
  return check_launch("mvp_edge_bn_relu_max_backward");
}
