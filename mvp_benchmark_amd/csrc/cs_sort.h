// The Morton index: a cloud's points in the order of 16^3 cells, with bounding boxes over runs of that order.  It is
// behind the three pruned exact searches -- chamfer.hip (nearest neighbour), pn2_query.hip (k nearest), fps.hip
// (furthest point sampling) -- and is built by cs_sort.hip into caller-provided scratch.
//
// Cells and order.  The cloud's bounding box [lo, lo + ext]^3 (ext = its largest extent; 1 when that is 0, subnormal-
// small, infinite or NaN) is cut into 16 x 16 x 16 cells, a point's cell per axis is (int)clamp((x - lo) * (16 / ext),
// 0, 15) -- NaN lands in cell 0, +-inf in 0 / 15 -- and cells are numbered by interleaving the three 4-bit indices
// (x in bits 0, 3, 6, 9).  One workgroup sorts one cloud by cell with a counting sort in LDS.  The order INSIDE a cell
// is whatever the LDS atomics gave: it differs from run to run, and no consumer may depend on it.
// An entry is float4 {x, y, z, bits(original index)}, the coordinates bitwise the input's.
//
// Layout, two conventions:
//   * a "side" (Chamfer, kNN; struct CsSide): cs_round_up(c) entries, the padding {+inf, +inf, +inf, kCsPad}; then the
//     box {lo, hi} (two float4, .w = 0) of every "tile" of 16 consecutive entries; then of every "batch" of 1024.
//     Padding is in no box; a tile of padding only has the empty box {+inf, -inf}.  A cloud pair's two sides follow
//     each other: cs_side_bytes(n1) + cs_side_bytes(n2) bytes per cloud.
//   * points only (FPS): npad entries per cloud, the padding {0, 0, 0, -1}; no boxes (fps_sorted_kernel keeps one box
//     per lane in registers).
//
// Exactness of the box tests.  cs_box_dist / cs_point_box_dist run sqdist3's subtract / fma chain on per-axis gaps
// that are <= every member pair's |difference|; float subtract, multiply and fma are monotone, so the box distance
// never exceeds a member pair's computed distance.  A search skips a box only on strict `>` against its current bound:
// a candidate that EQUALS the bound is still evaluated, and the result is the exhaustive search's.
#pragma once
#include "common.h"
#include "wave.h"

namespace mvp {

constexpr int kCsThreads = 1024;
constexpr int kCsCells = 4096;  // 16^3
constexpr int kCsTile = 16;
constexpr int kCsBatch = 1024;
constexpr int kCsPad = 0x7fffffff;  // original index of a side's padding entry

__host__ __device__ inline long long cs_round_up(long long c) { return (c + kCsBatch - 1) / kCsBatch * kCsBatch; }
// bytes of one sorted side holding c points: points + tile boxes + batch boxes
__host__ __device__ inline long long cs_side_bytes(long long c) {
  const long long cp = cs_round_up(c);
  return cp * 16 + cp / kCsTile * 32 + cp / kCsBatch * 32;
}

struct CsSide {
  float4 *pts;   // cp sorted points
  float4 *tbox;  // 2 per tile: lo, hi
  float4 *bbox;  // 2 per batch: lo, hi
};
__host__ __device__ inline CsSide cs_carve(char *base, long long c) {
  const long long cp = cs_round_up(c);
  CsSide s;
  s.pts = reinterpret_cast<float4 *>(base);
  s.tbox = reinterpret_cast<float4 *>(base + cp * 16);
  s.bbox = reinterpret_cast<float4 *>(base + cp * 16 + cp / kCsTile * 32);
  return s;
}

// ---- the frame of a pruned search over a side (a lane owns a query, a wave's 64 consecutive sorted queries sit in a
// small box -- wave_box of wave.h --, candidates stream through LDS one batch at a time)

// squared distance between two axis-aligned boxes (0 if they overlap)
__device__ __forceinline__ float cs_box_dist(const float (&qlo)[3], const float (&qhi)[3],
                                             const float4 &tlo, const float4 &thi) {
  const float gx = __builtin_fmaxf(__builtin_fmaxf(tlo.x - qhi[0], qlo[0] - thi.x), 0.f);
  const float gy = __builtin_fmaxf(__builtin_fmaxf(tlo.y - qhi[1], qlo[1] - thi.y), 0.f);
  const float gz = __builtin_fmaxf(__builtin_fmaxf(tlo.z - qhi[2], qlo[2] - thi.z), 0.f);
  return sqdist3(gx, gy, gz);
}
// the same between a point and a box
__device__ __forceinline__ float cs_point_box_dist(float x, float y, float z, const float4 &tlo, const float4 &thi) {
  const float gx = __builtin_fmaxf(__builtin_fmaxf(tlo.x - x, x - thi.x), 0.f);
  const float gy = __builtin_fmaxf(__builtin_fmaxf(tlo.y - y, y - thi.y), 0.f);
  const float gz = __builtin_fmaxf(__builtin_fmaxf(tlo.z - z, z - thi.z), 0.f);
  return sqdist3(gx, gy, gz);
}
// k-th batch of the outward order b0, b0+1, b0-1, b0+2, ... (b0: the query block's own relative position in the
// candidates' order, so the bounds are tight after the first batch or two); may fall outside [0, nb)
__device__ __forceinline__ int cs_batch_at(int b0, int k) { return b0 + ((k & 1) ? (k + 1) / 2 : -(k / 2)); }

// Sorts both sides of every cloud pair: xyz1 (b, n1, 3) -> side 0, xyz2 (b, n2, 3) -> side 1 of the cloud's scratch
// area.
void cs_sort_launch(int b, int n1, int n2, const float *xyz1, const float *xyz2, char *scratch, hipStream_t stream);
// Sorts every cloud of xyz (b, n, 3) into `sorted` (b, npad), points only.
void cs_sort_points_launch(int b, int n, int npad, const float *xyz, float4 *sorted, hipStream_t stream);

}  // namespace mvp
