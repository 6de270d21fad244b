// DeepGMR (registration/models/deepgmr.py): rotation-reference-invariant (RRI) point features and the moments of
// the soft Gaussian mixture, with its backward pass.
//
// RRI (replaces get_rri_cluster, reference registration/models/deepgmr.py:54-96).  The reference computes rp, rq,
// theta in torch, then moves T_q and p/|p| to the host and forms the (B*M, S, k, k, 3) cross / dot products, atan2,
// the remainder and an argpartition in NumPy.  Here one launch: a workgroup owns 64 points of one cloud (lane =
// point, so every store of the (b, 4k, n) output is 64 consecutive floats along n) and its 4 waves split the k
// neighbour slots.  Phase 1: each (point, slot) computes rq, theta and the tangent T_a and parks T_a in LDS as
// [slot][component][lane] (k * 3 * 64 floats of dynamic LDS: 15 KiB at k = 20, 48 KiB at k = 64).  Phase 2: each
// (point, slot a) walks all k slots b, reading T_b from LDS (lane-contiguous: conflict-free), and keeps the two
// smallest psi[a, b] -- phi_a is the second smallest of that multiset, psi[a, a] = 0 included
// (np.argpartition(psi, 1)[..., 1]).  k^2 atan2 per point.  A point at the origin (|p| = 0) or a neighbour there
// (|q_a| = 0) has no direction: theta and phi of the affected slots are NaN, as in the reference (see mvpops.h).
//
// GMM moments (replace gmm_params, deepgmr.py:98-121, and the softmax of Model.forward, :231-234).  Two launches
// for the forward pass: the softmax over j per point (grid over n-chunks x clouds), then one workgroup per
// (component, cloud) that reduces pi and mu over the cloud's n points and, in a second pass over the same points,
// the centred second moment sigma (two-pass, as the reference).  Every sum has a fixed order (per-thread strided
// partial, then a fixed tree over the workgroup): results are bit-identical from run to run, no atomics.  The
// backward pass is one elementwise launch (closed form, see include/mvpops.h).
#include "common.h"

namespace mvp {

constexpr int kRriMaxK = 64;
constexpr int kRriWaves = 4;
constexpr int kGmmMaxJ = 64;
constexpr int kGmmThreads = 256;

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
  return (ax * bx + ay * by) + az * bz;
}

__global__ __launch_bounds__(kWave *kRriWaves) void rri_features_kernel(int n, int k, const float *__restrict__ xyz,
                                                                          const int *__restrict__ idx,
                                                                          float *__restrict__ feat) {
  extern __shared__ float T[];  // k * 3 * 64 floats
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int cloud = blockIdx.y;
  const int i = blockIdx.x * kWave + lane;
  const bool valid = i < n;
  const int ic = valid ? i : n - 1;  // tail lanes compute on a real point and store nothing
  const float *pts = xyz + (size_t)cloud * n * 3;
  const int *nbr = idx + ((size_t)cloud * n + ic) * k;
  float *out = feat + (size_t)cloud * 4 * k * n + i;

  const float px = pts[ic * 3 + 0], py = pts[ic * 3 + 1], pz = pts[ic * 3 + 2];
  const float rp = sqrtf(dot3(px, py, pz, px, py, pz));
  const float pnx = px / rp, pny = py / rp, pnz = pz / rp;

  for (int a = wave; a < k; a += kRriWaves) {
    int j = nbr[a];
    j = (unsigned)j < (unsigned)n ? j : 0;  // stay inside the cloud whatever the index says
    const float qx = pts[j * 3 + 0], qy = pts[j * 3 + 1], qz = pts[j * 3 + 2];
    const float rq = sqrtf(dot3(qx, qy, qz, qx, qy, qz));
    const float d = dot3(pnx, pny, pnz, qx / rq, qy / rq, qz / rq);
    // clamp that keeps a NaN (fmaxf / fminf return their non-NaN operand and would turn it into acos(-1) = pi):
    // a point or a neighbour at the origin has no direction, theta is NaN as in the reference's torch.clamp
    const float theta = acosf(d < -1.0f ? -1.0f : d > 1.0f ? 1.0f : d);
    // T_a = q - (p^ . q^) p: the unclamped dot and the unnormalised p, as the reference writes it
    T[(a * 3 + 0) * kWave + lane] = qx - d * px;
    T[(a * 3 + 1) * kWave + lane] = qy - d * py;
    T[(a * 3 + 2) * kWave + lane] = qz - d * pz;
    if (valid) {
      out[(size_t)(4 * a + 0) * n] = rp;
      out[(size_t)(4 * a + 1) * n] = rq;
      out[(size_t)(4 * a + 2) * n] = theta;
    }
  }
  __syncthreads();

  const float kTwoPi = 6.2831855f;  // float32(2 pi): the remainder of the reference runs on float32 arrays
  for (int a = wave; a < k; a += kRriWaves) {
    const float ax = T[(a * 3 + 0) * kWave + lane], ay = T[(a * 3 + 1) * kWave + lane],
                az = T[(a * 3 + 2) * kWave + lane];
    float m1 = INFINITY, m2 = INFINITY;
    for (int b = 0; b < k; ++b) {
      const float bx = T[(b * 3 + 0) * kWave + lane], by = T[(b * 3 + 1) * kWave + lane],
                  bz = T[(b * 3 + 2) * kWave + lane];
      // sin psi = (T_b x T_a) . p^, cos psi = T_b . T_a (np.cross(T_q[:, :, None], T_q[:, :, :, None]))
      const float cx = by * az - bz * ay, cy = bz * ax - bx * az, cz = bx * ay - by * ax;
      const float s = dot3(cx, cy, cz, pnx, pny, pnz);
      const float c = dot3(bx, by, bz, ax, ay, az);
      float psi = atan2f(s, c);
      // np.remainder(psi, 2 pi) for |psi| <= pi: psi + 2 pi below zero (may round to 2 pi itself), +0 for -0
      psi = psi < 0.0f ? psi + kTwoPi : psi + 0.0f;
      if (psi < m1) {
        m2 = m1;
        m1 = psi;
      } else if (psi < m2) {
        m2 = psi;
      }
    }
    // every finite psi is <= 2 pi, so m2 is still +inf only when the row holds fewer than two non-NaN psi (the
    // point or all but one tangent undefined): NaN, as the reference's sort, which puts NaN last
    if (valid) out[(size_t)(4 * a + 3) * n] = m2 == INFINITY ? NAN : m2;
  }
}

// Softmax over j of logits (b, j, n) -> gamma (b, n, j): max-subtracted, sum in j order.
__global__ __launch_bounds__(kGmmThreads) void gmm_softmax_kernel(int n, int j, const float *__restrict__ logits,
                                                                  float *__restrict__ gamma) {
  const int cloud = blockIdx.y;
  const int i = blockIdx.x * kGmmThreads + threadIdx.x;
  if (i >= n) return;
  const float *l = logits + (size_t)cloud * j * n + i;
  float m = -INFINITY;
  for (int c = 0; c < j; ++c) m = fmaxf(m, l[(size_t)c * n]);
  float s = 0.0f;
  for (int c = 0; c < j; ++c) s += expf(l[(size_t)c * n] - m);
  float *g = gamma + ((size_t)cloud * n + i) * j;
  for (int c = 0; c < j; ++c) g[c] = expf(l[(size_t)c * n] - m) / s;
}

// Fixed-order sum of one value per thread over the workgroup; every thread gets the total.
__device__ __forceinline__ float block_sum(float v, float *red) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  __syncthreads();  // red may still be read by the previous call
  if (lane == 0) red[wave] = v;
  __syncthreads();
  float t = red[0];
#pragma unroll
  for (int w = 1; w < kGmmThreads / kWave; ++w) t += red[w];
  return t;
}

// One workgroup per (component c, cloud): pi = mean_n gamma, mu = sum gamma p / (N pi),
// sigma = sum gamma |p - mu|^2 / (N pi).
__global__ __launch_bounds__(kGmmThreads) void gmm_moments_kernel(int n, int j, const float *__restrict__ xyz,
                                                                  const float *__restrict__ gamma,
                                                                  float *__restrict__ pi, float *__restrict__ mu,
                                                                  float *__restrict__ sigma) {
  __shared__ float red[kGmmThreads / kWave];
  const int c = blockIdx.x, cloud = blockIdx.y;
  const float *pts = xyz + (size_t)cloud * n * 3;
  const float *g = gamma + (size_t)cloud * n * j + c;
  float s0 = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
  for (int i = threadIdx.x; i < n; i += kGmmThreads) {
    const float w = g[(size_t)i * j];
    s0 += w;
    sx += w * pts[i * 3 + 0];
    sy += w * pts[i * 3 + 1];
    sz += w * pts[i * 3 + 2];
  }
  s0 = block_sum(s0, red);
  sx = block_sum(sx, red);
  sy = block_sum(sy, red);
  sz = block_sum(sz, red);
  const float p = s0 / (float)n, npi = p * (float)n;  // the reference's pi = gamma.mean(1), Npi = pi * N
  const float mx = sx / npi, my = sy / npi, mz = sz / npi;
  float s2 = 0.0f;
  for (int i = threadIdx.x; i < n; i += kGmmThreads) {
    const float dx = pts[i * 3 + 0] - mx, dy = pts[i * 3 + 1] - my, dz = pts[i * 3 + 2] - mz;
    s2 += g[(size_t)i * j] * dot3(dx, dy, dz, dx, dy, dz);
  }
  s2 = block_sum(s2, red);
  if (threadIdx.x == 0) {
    const size_t o = (size_t)cloud * j + c;
    pi[o] = p;
    mu[o * 3 + 0] = mx;
    mu[o * 3 + 1] = my;
    mu[o * 3 + 2] = mz;
    sigma[o] = s2 / npi;
  }
}

// g_logits[c][i] = gamma_ic (g_gamma_ic - sum_c' gamma_ic' g_gamma_ic'), one thread per point.
__global__ __launch_bounds__(kGmmThreads) void gmm_backward_kernel(
    int n, int j, const float *__restrict__ gamma, const float *__restrict__ xyz, const float *__restrict__ pi,
    const float *__restrict__ mu, const float *__restrict__ sigma, const float *__restrict__ g_pi,
    const float *__restrict__ g_mu, const float *__restrict__ g_sigma, float *__restrict__ g_logits) {
  // per component: g_pi / N, g_mu / (N pi) (3), mu (3), sigma, g_sigma / (N pi)
  __shared__ float par[kGmmMaxJ][9];
  const int cloud = blockIdx.y;
  for (int c = threadIdx.x; c < j; c += kGmmThreads) {
    const size_t o = (size_t)cloud * j + c;
    const float npi = pi[o] * (float)n;
    par[c][0] = g_pi[o] / (float)n;
    par[c][1] = g_mu[o * 3 + 0] / npi;
    par[c][2] = g_mu[o * 3 + 1] / npi;
    par[c][3] = g_mu[o * 3 + 2] / npi;
    par[c][4] = mu[o * 3 + 0];
    par[c][5] = mu[o * 3 + 1];
    par[c][6] = mu[o * 3 + 2];
    par[c][7] = sigma[o];
    par[c][8] = g_sigma[o] / npi;
  }
  __syncthreads();
  const int i = blockIdx.x * kGmmThreads + threadIdx.x;
  if (i >= n) return;
  const float *p = xyz + ((size_t)cloud * n + i) * 3;
  const float px = p[0], py = p[1], pz = p[2];
  const float *g = gamma + ((size_t)cloud * n + i) * j;
  float *gl = g_logits + (size_t)cloud * j * n + i;
  auto g_gamma = [&](int c) {
    const float dx = px - par[c][4], dy = py - par[c][5], dz = pz - par[c][6];
    return (par[c][0] + dot3(par[c][1], par[c][2], par[c][3], dx, dy, dz)) +
           par[c][8] * (dot3(dx, dy, dz, dx, dy, dz) - par[c][7]);
  };
  float dot = 0.0f;
  for (int c = 0; c < j; ++c) dot += g[c] * g_gamma(c);
  for (int c = 0; c < j; ++c) gl[(size_t)c * n] = g[c] * (g_gamma(c) - dot);
}

}  // namespace mvp

using namespace mvp;

extern "C" int mvp_rri_features(int b, int n, int k, const float *xyz, const int *idx, float *feat, void *stream) {
  if (b < 0 || n < 0) return MVP_EBADSHAPE;
  if (k < 2 || k > kRriMaxK) return MVP_EBADARG;  // k < 2: the reference's argpartition(psi, 1) has no second slot
  if (b == 0 || n == 0) return MVP_OK;
  if (!xyz || !idx || !feat) return MVP_EBADARG;
  hipLaunchKernelGGL(rri_features_kernel, dim3((n + kWave - 1) / kWave, b), dim3(kWave * kRriWaves),
                     (size_t)k * 3 * kWave * sizeof(float), as_stream(stream), n, k, xyz, idx, feat);
  return check_launch("mvp_rri_features");
}

extern "C" int mvp_gmm_params(int b, int n, int j, const float *logits, const float *xyz, float *gamma, float *pi,
                              float *mu, float *sigma, void *stream) {
  if (b < 0 || n < 1) return MVP_EBADSHAPE;
  if (j < 1 || j > kGmmMaxJ) return MVP_EBADARG;
  if (b == 0) return MVP_OK;
  if (!logits || !xyz || !gamma || !pi || !mu || !sigma) return MVP_EBADARG;
  hipLaunchKernelGGL(gmm_softmax_kernel, dim3((n + kGmmThreads - 1) / kGmmThreads, b), dim3(kGmmThreads), 0,
                     as_stream(stream), n, j, logits, gamma);
  int rc = check_launch("mvp_gmm_params");
  if (rc != MVP_OK) return rc;
  hipLaunchKernelGGL(gmm_moments_kernel, dim3(j, b), dim3(kGmmThreads), 0, as_stream(stream), n, j, xyz, gamma, pi,
                     mu, sigma);
  return check_launch("mvp_gmm_params");
}

extern "C" int mvp_gmm_params_backward(int b, int n, int j, const float *gamma, const float *xyz, const float *pi,
                                       const float *mu, const float *sigma, const float *g_pi, const float *g_mu,
                                       const float *g_sigma, float *g_logits, void *stream) {
  if (b < 0 || n < 1) return MVP_EBADSHAPE;
  if (j < 1 || j > kGmmMaxJ) return MVP_EBADARG;
  if (b == 0) return MVP_OK;
  if (!gamma || !xyz || !pi || !mu || !sigma || !g_pi || !g_mu || !g_sigma || !g_logits) return MVP_EBADARG;
  hipLaunchKernelGGL(gmm_backward_kernel, dim3((n + kGmmThreads - 1) / kGmmThreads, b), dim3(kGmmThreads), 0,
                     as_stream(stream), n, j, gamma, xyz, pi, mu, sigma, g_pi, g_mu, g_sigma, g_logits);
  return check_launch("mvp_gmm_params_backward");
}
