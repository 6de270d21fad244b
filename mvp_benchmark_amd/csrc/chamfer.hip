// Chamfer distance for gfx950: bidirectional nearest-neighbour squared
// distance + arg-min (forward) and its gradient (backward).
//
// Replaces NmDistanceKernel / NmDistanceGradKernel of the reference
// (utils/metrics/CD/chamfer3D/chamfer3D.cu:12-134,155-174).  Not a port: the
// reference stages 512-point tiles and tracks (best, best_i) per candidate in
// a fixed 32x16 grid.  Here
//   * both directions run in ONE launch (blockIdx.z), sized to the problem so
//     every cloud/query block gets its own workgroup (>> 256 workgroups);
//   * each lane owns Q query points in registers and streams candidate points
//     from an LDS tile with wave-uniform ds_read_b128 (broadcast, no bank
//     conflicts): 3 reads deliver 4 candidates;
//   * the hot loop only tracks the running MINIMUM over sub-tiles of 16
//     candidates (v_min), remembering which sub-tile last lowered it; the
//     arg-min is recovered afterwards by re-scanning that single sub-tile
//     ("min-then-locate").  This removes the compare+2 selects per pair that
//     index tracking costs, and keeps the reference's tie rule exactly:
//     strict `<` between sub-tiles (earliest sub-tile wins) and first equal
//     candidate inside it (lowest index wins) -- chamfer3D.cu:36,46,126.
//   * arithmetic is the canonical fma chain shared with the CPU oracle.
#include "common.h"
#include "cs_sort.h"

namespace mvp {

constexpr int kCdThreads = 256;
constexpr int kCdTile = 1024;  // candidates per LDS tile (12 KiB)
constexpr int kCdSub = 16;     // candidates per min-tracking sub-tile
// Distance written for a query whose distances are ALL NaN (index 0 with it):
// the quiet, positive NaN, whatever payload the arithmetic produced.
constexpr unsigned kCdNanBits = 0x7fc00000u;
constexpr unsigned kCdInfBits = 0x7f800000u;

template <int Q>
__global__ __launch_bounds__(kCdThreads) void nm_distance_kernel(
    int n1, int n2, const float *__restrict__ xyz1,
    const float *__restrict__ xyz2, float *__restrict__ dist1,
    float *__restrict__ dist2, int *__restrict__ idx1, int *__restrict__ idx2) {
  // Direction 0: queries = xyz1 (n1 points), candidates = xyz2 (n2 points).
  // Direction 1: roles swapped.
  const int dir = blockIdx.z;
  const int n = dir == 0 ? n1 : n2;
  const int m = dir == 0 ? n2 : n1;
  if ((int)blockIdx.x * (kCdThreads * Q) >= n) return;
  const int cloud = blockIdx.y;
  const float *__restrict__ qpts = (dir == 0 ? xyz1 : xyz2) + (size_t)cloud * n * 3;
  const float *__restrict__ cpts = (dir == 0 ? xyz2 : xyz1) + (size_t)cloud * m * 3;
  float *__restrict__ result = (dir == 0 ? dist1 : dist2) + (size_t)cloud * n;
  int *__restrict__ result_i = (dir == 0 ? idx1 : idx2) + (size_t)cloud * n;

  __shared__ __attribute__((aligned(16))) float tile[kCdTile * 3];

  const int tid = threadIdx.x;
  float qx[Q], qy[Q], qz[Q], best[Q];
  int bsub[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    int j = blockIdx.x * (kCdThreads * Q) + q * kCdThreads + tid;
    j = j < n ? j : n - 1;
    qx[q] = qpts[j * 3 + 0];
    qy[q] = qpts[j * 3 + 1];
    qz[q] = qpts[j * 3 + 2];
    best[q] = __builtin_inff();
    bsub[q] = 0;
  }

  for (int k2 = 0; k2 < m; k2 += kCdTile) {
    const int cnt = min(kCdTile, m - k2);
    // Stage the tile (AoS, exactly as in global memory); pad the tail of the
    // last sub-tile with +inf so padded candidates evaluate to d = +inf.
    const int padded = ((cnt + kCdSub - 1) / kCdSub) * kCdSub;
    for (int t = tid; t < padded * 3; t += kCdThreads)
      tile[t] = t < cnt * 3 ? cpts[(size_t)k2 * 3 + t] : __builtin_inff();
    __syncthreads();

    const float4 *__restrict__ t4 = reinterpret_cast<const float4 *>(tile);
    const int nsub = padded / kCdSub;
    for (int s = 0; s < nsub; ++s) {
      float tmin[Q];
#pragma unroll
      for (int q = 0; q < Q; ++q) tmin[q] = __builtin_inff();
#pragma unroll
      for (int g = 0; g < kCdSub / 4; ++g) {
        const float4 a = t4[(s * (kCdSub / 4) + g) * 3 + 0];
        const float4 b = t4[(s * (kCdSub / 4) + g) * 3 + 1];
        const float4 c = t4[(s * (kCdSub / 4) + g) * 3 + 2];
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          const float d0 = sqdist3(a.x - qx[q], a.y - qy[q], a.z - qz[q]);
          const float d1 = sqdist3(a.w - qx[q], b.x - qy[q], b.y - qz[q]);
          const float d2 = sqdist3(b.z - qx[q], b.w - qy[q], c.x - qz[q]);
          const float d3 = sqdist3(c.y - qx[q], c.z - qy[q], c.w - qz[q]);
          tmin[q] = __builtin_fminf(__builtin_fminf(tmin[q], d0), d1);
          tmin[q] = __builtin_fminf(__builtin_fminf(tmin[q], d2), d3);
        }
      }
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const bool lower = tmin[q] < best[q];
        best[q] = lower ? tmin[q] : best[q];
        bsub[q] = lower ? (k2 / kCdSub + s) : bsub[q];
      }
    }
    __syncthreads();
  }

  // Locate: first candidate of the winning sub-tile whose distance equals the
  // minimum (bitwise-identical recomputation).
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int j = blockIdx.x * (kCdThreads * Q) + q * kCdThreads + tid;
    if (j >= n) continue;
    const int k0 = bsub[q] * kCdSub;
    const int k1 = min(k0 + kCdSub, m);
    int bi = k0;
    bool found = false;
    for (int k = k0; k < k1; ++k) {
      const float d = sqdist3(cpts[k * 3 + 0] - qx[q], cpts[k * 3 + 1] - qy[q],
                              cpts[k * 3 + 2] - qz[q]);
      if (!found && d == best[q]) {
        bi = k;
        found = true;
      }
    }
    float bd = best[q];
    if (bd == __builtin_inff()) {
      // No finite distance (overflowing squares, non-finite coordinates): fminf
      // dropped every NaN and no sub-tile ever lowered `best`, so `bsub` says
      // nothing.  +inf is a value like any other -- the first candidate at +inf
      // wins -- and a query whose distances are all NaN gets (NaN, 0).  Rare and
      // per lane, hence a plain scan of the query's candidates.
      bd = __uint_as_float(kCdNanBits);
      bi = 0;
      for (int k = 0; k < m; ++k) {
        const float d = sqdist3(cpts[k * 3 + 0] - qx[q], cpts[k * 3 + 1] - qy[q],
                                cpts[k * 3 + 2] - qz[q]);
        if (d == __builtin_inff()) {
          bd = d;
          bi = k;
          break;
        }
      }
    }
    result[j] = bd;
    result_i[j] = bi;
  }
}

// ---------------------------------------------------------------------------
// Spatially sorted variant for large clouds: the same result with most of the
// B*N*M pairs never evaluated.  Both sides are Morton-sorted with boxes per
// tile and per batch (cs_sort.h: the index, the frame of a pruned search and
// why the box tests are exact).  nm_distance_sorted_kernel keeps the
// brute-force skeleton -- a lane owns a query, candidates stream through LDS
// batches -- and skips a tile / batch when the distance between the box of the
// wave's 64 queries and the tile's box already exceeds the worst current best
// of the wave.  Ties go to the lowest ORIGINAL index (chamfer3D.cu:36,46,126)
// by minimising the key {distance bits, original index} -- the visiting order
// no longer is the index order.
__global__ __launch_bounds__(kCdThreads) void nm_distance_sorted_kernel(
    int n1, int n2, char *__restrict__ scratch, float *__restrict__ dist1,
    float *__restrict__ dist2, int *__restrict__ idx1, int *__restrict__ idx2) {
  const int dir = blockIdx.z;
  const int nq = dir == 0 ? n1 : n2;
  const int nc = dir == 0 ? n2 : n1;
  if ((int)blockIdx.x * kCdThreads >= nq) return;
  const int cloud = blockIdx.y;
  const long long per_cloud = cs_side_bytes(n1) + cs_side_bytes(n2);
  char *cbase = scratch + (size_t)cloud * per_cloud;
  const CsSide s1 = cs_carve(cbase, n1), s2 = cs_carve(cbase + cs_side_bytes(n1), n2);
  const CsSide qs = dir == 0 ? s1 : s2, cs = dir == 0 ? s2 : s1;
  float *__restrict__ result = (dir == 0 ? dist1 : dist2) + (size_t)cloud * nq;
  int *__restrict__ result_i = (dir == 0 ? idx1 : idx2) + (size_t)cloud * nq;

  __shared__ __attribute__((aligned(16))) float4 tile[kCsBatch];
  __shared__ __attribute__((aligned(16))) float4 tbx[2 * kCsBatch / kCsTile];

  const int tid = threadIdx.x;
  // a wave's 64 queries are consecutive in the sorted order (a compact box)
  int j = blockIdx.x * kCdThreads + tid;
  const bool valid = j < nq;
  j = valid ? j : nq - 1;
  const float4 qp = qs.pts[j];
  const float qx = qp.x, qy = qp.y, qz = qp.z;
  const int qorig = valid ? __float_as_int(qp.w) : -1;
  unsigned long long best = ~0ull;
  const float inf = __builtin_inff();
  float qlo[3] = {__builtin_fminf(inf, qx), __builtin_fminf(inf, qy), __builtin_fminf(inf, qz)};  // (a NaN stays out of the box)
  float qhi[3] = {__builtin_fmaxf(-inf, qx), __builtin_fmaxf(-inf, qy), __builtin_fmaxf(-inf, qz)};
  wave_box(qlo, qhi);
  float wmax = __builtin_inff();  // worst current best distance in this wave

  const int nb = (int)(cs_round_up(nc) / kCsBatch);
  const int nblk = (nq + kCdThreads - 1) / kCdThreads;
  const int b0 = (int)((long long)blockIdx.x * nb / nblk);  // same relative position in the order
  for (int k = 0; k < 2 * nb; ++k) {
    const int bi = cs_batch_at(b0, k);
    if (bi < 0 || bi >= nb) continue;                        // block-uniform
    const bool need = !(cs_box_dist(qlo, qhi, cs.bbox[2 * bi], cs.bbox[2 * bi + 1]) > wmax);  // wave-uniform
    if (!__syncthreads_or(need)) continue;
    for (int i = tid; i < kCsBatch; i += kCdThreads) tile[i] = cs.pts[(size_t)bi * kCsBatch + i];
    if (tid < 2 * kCsBatch / kCsTile) tbx[tid] = cs.tbox[(size_t)bi * (2 * kCsBatch / kCsTile) + tid];
    __syncthreads();
    if (need) {
      // lane l tests tile l of the batch (64 tiles); the survivors are visited
      // in order and re-tested against the bests as they tighten
      const float lbl = cs_box_dist(qlo, qhi, tbx[2 * (tid & 63)], tbx[2 * (tid & 63) + 1]);
      // Round 6: the tiles whose box OVERLAPS the wave's query box first -- they hold the queries' neighbourhoods, so the
      // worst best of the wave is tight before the others are tested against it (in index order the first tiles of a
      // batch were evaluated against wmax = inf whether near or far): (64, 16384 x 16384) 0.96 -> 0.81 ms.  (Strictly
      // nearest-first -- a wave minimum per visit -- costs what it saves: 0.94; the decision per 16-lane row: 1.11.)
      const unsigned long long all = __ballot(!(lbl > wmax));
      unsigned long long near = __ballot(lbl == 0.f) & all;
      unsigned long long todo = all & ~near;
      while (near | todo) {
        unsigned long long &from = near ? near : todo;
        const int s = __builtin_ctzll(from);
        from &= from - 1;
        if (read_lane(lbl, s) > wmax) continue;
        // precise test: does ANY query of the wave still need this tile?  (the query POINT against the tile's box
        // and that query's own best)
        const float mybest = __uint_as_float((unsigned)(best >> 32));
        if (!__any(!(cs_point_box_dist(qx, qy, qz, tbx[2 * s], tbx[2 * s + 1]) > mybest))) continue;
#pragma unroll
        for (int c = 0; c < kCsTile; ++c) {
          const float4 p = tile[s * kCsTile + c];
          const float d = sqdist3(p.x - qx, p.y - qy, p.z - qz);
          const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | __float_as_uint(p.w);
          best = key < best ? key : best;
        }
        wmax = wave_max(__uint_as_float((unsigned)(best >> 32)));
      }
    }
    __syncthreads();
  }
  if (qorig >= 0) {
    // NaN bits sort above +inf, so a NaN key is the minimum only when every
    // distance of the query is NaN; a padding entry (+inf coordinates) is the
    // minimum only when every real candidate's distance is: both are the
    // "all NaN" query of the contract, written as (NaN, 0) like the
    // exhaustive kernel does.
    unsigned dbits = (unsigned)(best >> 32);
    int bi = (int)(unsigned)best;
    if (dbits > kCdInfBits || bi == kCsPad) {
      dbits = kCdNanBits;
      bi = 0;
    }
    result[qorig] = __uint_as_float(dbits);
    result_i[qorig] = bi;
  }
}


// Gradient.  One thread per (cloud, point); both directions in one launch.
// grad_xyzA[j] += 2 g (a_j - b_idx), grad_xyzB[idx] -= same (float atomics,
// accumulation order unspecified as in the reference).
__global__ __launch_bounds__(256) void nm_distance_grad_kernel(
    int n1, int n2, const float *__restrict__ xyz1,
    const float *__restrict__ xyz2, const float *__restrict__ graddist1,
    const float *__restrict__ graddist2, const int *__restrict__ idx1,
    const int *__restrict__ idx2, float *__restrict__ gradxyz1,
    float *__restrict__ gradxyz2) {
  const int dir = blockIdx.z;
  const int n = dir == 0 ? n1 : n2;
  const int m = dir == 0 ? n2 : n1;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int cloud = blockIdx.y;
  const float *a = (dir == 0 ? xyz1 : xyz2) + ((size_t)cloud * n + j) * 3;
  const int j2 = (dir == 0 ? idx1 : idx2)[(size_t)cloud * n + j];
  const float *c = (dir == 0 ? xyz2 : xyz1) + ((size_t)cloud * m + j2) * 3;
  const float g = (dir == 0 ? graddist1 : graddist2)[(size_t)cloud * n + j] * 2;
  float *ga = (dir == 0 ? gradxyz1 : gradxyz2) + ((size_t)cloud * n + j) * 3;
  float *gc = (dir == 0 ? gradxyz2 : gradxyz1) + ((size_t)cloud * m + j2) * 3;
  const float gx = g * (a[0] - c[0]);
  const float gy = g * (a[1] - c[1]);
  const float gz = g * (a[2] - c[2]);
  atomicAdd(ga + 0, gx);
  atomicAdd(ga + 1, gy);
  atomicAdd(ga + 2, gz);
  atomicAdd(gc + 0, -gx);
  atomicAdd(gc + 1, -gy);
  atomicAdd(gc + 2, -gz);
}

// The same gradient for training-size clouds (n + m <= 8192 points): one
// workgroup per cloud accumulates both gradient arrays in LDS -- a point's own
// term with a plain add, the scattered term with ds_add_f32 -- and adds the
// result to the (zero-filled) outputs with coalesced, non-atomic writes.  Six
// global float atomics per point (each a full L2 read-modify-write; nearest
// neighbours collide) become six LDS operations: (64, 2048, 2048) 0.19 ->
// 0.03 ms.
constexpr int kCgThreads = 1024;
constexpr int kCgMaxPoints = 8192;  // (n + m) * 12 B of LDS

__global__ __launch_bounds__(kCgThreads) void nm_distance_grad_lds_kernel(
    int n1, int n2, const float *__restrict__ xyz1, const float *__restrict__ xyz2,
    const float *__restrict__ graddist1, const float *__restrict__ graddist2, const int *__restrict__ idx1,
    const int *__restrict__ idx2, float *__restrict__ gradxyz1, float *__restrict__ gradxyz2) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float *acc1 = reinterpret_cast<float *>(smem);  // n1 * 3
  float *acc2 = acc1 + (size_t)n1 * 3;            // n2 * 3
  const int t = threadIdx.x;
  const int cloud = blockIdx.x;
  xyz1 += (size_t)cloud * n1 * 3;
  xyz2 += (size_t)cloud * n2 * 3;
  for (int i = t; i < (n1 + n2) * 3; i += kCgThreads) acc1[i] = 0.f;
  __syncthreads();
  for (int dir = 0; dir < 2; ++dir) {
    const int n = dir == 0 ? n1 : n2;
    const float *pa = dir == 0 ? xyz1 : xyz2;
    const float *pc = dir == 0 ? xyz2 : xyz1;
    const float *gd = (dir == 0 ? graddist1 : graddist2) + (size_t)cloud * n;
    const int *id = (dir == 0 ? idx1 : idx2) + (size_t)cloud * n;
    float *own = dir == 0 ? acc1 : acc2;
    float *oth = dir == 0 ? acc2 : acc1;
    for (int j = t; j < n; j += kCgThreads) {
      const int j2 = id[j];
      const float g = gd[j] * 2;
      const float gx = g * (pa[j * 3 + 0] - pc[j2 * 3 + 0]);
      const float gy = g * (pa[j * 3 + 1] - pc[j2 * 3 + 1]);
      const float gz = g * (pa[j * 3 + 2] - pc[j2 * 3 + 2]);
      // `own[j]` is also a scatter target of the other direction, which runs
      // in the other pass of this loop (separated by the barrier below)
      own[j * 3 + 0] += gx;
      own[j * 3 + 1] += gy;
      own[j * 3 + 2] += gz;
      atomicAdd(&oth[j2 * 3 + 0], -gx);
      atomicAdd(&oth[j2 * 3 + 1], -gy);
      atomicAdd(&oth[j2 * 3 + 2], -gz);
    }
    __syncthreads();
  }
  float *o1 = gradxyz1 + (size_t)cloud * n1 * 3;
  float *o2 = gradxyz2 + (size_t)cloud * n2 * 3;
  for (int i = t; i < n1 * 3; i += kCgThreads) o1[i] += acc1[i];
  for (int i = t; i < n2 * 3; i += kCgThreads) o2[i] += acc2[i];
}

}  // namespace mvp

using namespace mvp;

template <int Q>   // queries per lane; both directions in one launch, sized by the larger side
static void nm_distance_launch(int b, int n, int m, const float *xyz1, const float *xyz2, float *dist1, float *dist2,
                               int *idx1, int *idx2, hipStream_t stream) {
  const int big = n > m ? n : m;
  dim3 grid((big + kCdThreads * Q - 1) / (kCdThreads * Q), b, 2);
  hipLaunchKernelGGL(nm_distance_kernel<Q>, grid, dim3(kCdThreads), 0, stream, n, m, xyz1, xyz2, dist1, dist2, idx1,
                     idx2);
}

extern "C" int mvp_chamfer_forward(int b, int n, int m, const float *xyz1,
                                   const float *xyz2, float *dist1,
                                   float *dist2, int *idx1, int *idx2,
                                   void *stream) {
  if (b < 0 || n < 0 || m < 0) return MVP_EBADSHAPE;
  if (b == 0 || (n == 0 && m == 0)) return MVP_OK;
  if (n == 0 || m == 0) return MVP_EBADSHAPE;  // no nearest neighbour exists
  if (!xyz1 || !xyz2 || !dist1 || !dist2 || !idx1 || !idx2) return MVP_EBADARG;
  if (b > 65535) return MVP_EBADSHAPE;
  // Q queries per lane: 4 when there is enough work to fill 256 CUs anyway.
  const long long work = (long long)b * (n > m ? n : m);
  if (work >= 4LL * 256 * kCdThreads * 4)
    nm_distance_launch<4>(b, n, m, xyz1, xyz2, dist1, dist2, idx1, idx2, as_stream(stream));
  else if (work >= 2LL * 256 * kCdThreads * 2)
    nm_distance_launch<2>(b, n, m, xyz1, xyz2, dist1, dist2, idx1, idx2, as_stream(stream));
  else
    nm_distance_launch<1>(b, n, m, xyz1, xyz2, dist1, dist2, idx1, idx2, as_stream(stream));
  return check_launch("mvp_chamfer_forward");
}

extern "C" long long mvp_chamfer_scratch_bytes(int b, int n, int m) {
  if (b < 0 || n < 0 || m < 0) return -1;
  return (long long)b * (cs_side_bytes(n) + cs_side_bytes(m));
}

extern "C" int mvp_chamfer_forward_sorted(int b, int n, int m, const float *xyz1,
                                          const float *xyz2, float *dist1, float *dist2,
                                          int *idx1, int *idx2, void *scratch,
                                          long long scratch_bytes, void *stream) {
  // small clouds: the exhaustive kernel is already cheaper than sorting
  // (break-even measured at about 4096 x 4096 pairs per cloud)
  if (b <= 0 || n < 2048 || m < 2048 || (long long)n * m < (1ll << 24) || (n > m ? n : m) > (1 << 30))
    return mvp_chamfer_forward(b, n, m, xyz1, xyz2, dist1, dist2, idx1, idx2, stream);
  if (!xyz1 || !xyz2 || !dist1 || !dist2 || !idx1 || !idx2) return MVP_EBADARG;
  if (scratch_short(scratch, scratch_bytes, mvp_chamfer_scratch_bytes(b, n, m))) return MVP_EBADARG;
  if (b > 65535) return MVP_EBADSHAPE;
  cs_sort_launch(b, n, m, xyz1, xyz2, reinterpret_cast<char *>(scratch), as_stream(stream));
  // One query per lane: a wave's 64 consecutive sorted queries make the
  // smallest box, so the most tiles are skipped (measured: Q = 1 / 2 / 4 ->
  // 0.88 / 1.02 / 1.35 ms at (64, 16384, 16384); exhaustive 3.95 ms).
  const int big = n > m ? n : m;
  dim3 grid((big + kCdThreads - 1) / kCdThreads, b, 2);
  hipLaunchKernelGGL(nm_distance_sorted_kernel, grid, dim3(kCdThreads), 0, as_stream(stream), n, m,
                     reinterpret_cast<char *>(scratch), dist1, dist2, idx1, idx2);
  return check_launch("mvp_chamfer_forward_sorted");
}

extern "C" int mvp_chamfer_backward(int b, int n, int m, const float *xyz1,
                                    const float *xyz2, float *gradxyz1,
                                    float *gradxyz2, const float *graddist1,
                                    const float *graddist2, const int *idx1,
                                    const int *idx2, void *stream) {
  if (b < 0 || n < 0 || m < 0) return MVP_EBADSHAPE;
  if (b == 0 || (n == 0 && m == 0)) return MVP_OK;
  if (n == 0 || m == 0) return MVP_EBADSHAPE;
  if (!xyz1 || !xyz2 || !gradxyz1 || !gradxyz2 || !graddist1 || !graddist2 ||
      !idx1 || !idx2)
    return MVP_EBADARG;
  if (b > 65535) return MVP_EBADSHAPE;
  if (n + m <= kCgMaxPoints) {
    hipLaunchKernelGGL(nm_distance_grad_lds_kernel, dim3(b), dim3(kCgThreads), (size_t)(n + m) * 12, as_stream(stream),
                       n, m, xyz1, xyz2, graddist1, graddist2, idx1, idx2, gradxyz1, gradxyz2);
    return check_launch("mvp_chamfer_backward");
  }
  const int big = n > m ? n : m;
  dim3 grid((big + 255) / 256, b, 2);
  hipLaunchKernelGGL(nm_distance_grad_kernel, grid, dim3(256), 0,
                     as_stream(stream), n, m, xyz1, xyz2, graddist1, graddist2,
                     idx1, idx2, gradxyz1, gradxyz2);
  return check_launch("mvp_chamfer_backward");
}
