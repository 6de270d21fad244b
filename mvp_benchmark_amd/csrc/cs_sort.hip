// Builds the Morton index described in cs_sort.h: one workgroup of 1024 threads per cloud (and side), a counting sort
// over the 4096 cells in LDS, then -- for the side layout -- the tile and batch boxes.
#include "cs_sort.h"

namespace mvp {

__device__ __forceinline__ int cs_spread4(int v) {  // bit i -> bit 3i
  v &= 0xF;
  v = (v | (v << 4)) & 0xC3;
  v = (v | (v << 2)) & 0x249;
  return v;
}

// in (cnt, 3) -> out[0, cnt): {x, y, z, bits(original index)} in cell order; out[cnt, cp): `pad`.
__device__ __forceinline__ void cs_sort_points(const float *__restrict__ in, int cnt, float4 *__restrict__ out, int cp,
                                               float4 pad) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;

  __shared__ int s_cnt[kCsCells];
  __shared__ int s_start[kCsCells];
  __shared__ float s_red[6][kCsThreads / 64];
  __shared__ int s_wsum[kCsThreads / 64];

  // bounding box
  float mn[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
  float mx[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
  for (int k = t; k < cnt; k += kCsThreads) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float v = in[k * 3 + a];
      mn[a] = __builtin_fminf(mn[a], v);
      mx[a] = __builtin_fmaxf(mx[a], v);
    }
  }
  wave_box(mn, mx);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (lane == 0) {
      s_red[a][wave] = mn[a];
      s_red[3 + a][wave] = mx[a];
    }
  }
  for (int c = t; c < kCsCells; c += kCsThreads) s_cnt[c] = 0;
  __syncthreads();
  float lo[3], ext = 0.f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    float l = s_red[a][0], h = s_red[3 + a][0];
    for (int w = 1; w < kCsThreads / 64; ++w) {
      l = __builtin_fminf(l, s_red[a][w]);
      h = __builtin_fmaxf(h, s_red[3 + a][w]);
    }
    lo[a] = l;
    ext = __builtin_fmaxf(ext, h - l);
  }
  if (!(ext > 0.f) || !(ext < 3.0e38f)) ext = 1.f;
  const float invh = 16.f / ext;
  auto cell_of = [&](float x, float y, float z) {
    // clamped as floats: 0 * inf (a subnormal extent makes invh = +inf), a NaN
    // or an infinite coordinate must not reach the float -> int conversion
    const int ix = (int)__builtin_fminf(__builtin_fmaxf((x - lo[0]) * invh, 0.f), 15.f);
    const int iy = (int)__builtin_fminf(__builtin_fmaxf((y - lo[1]) * invh, 0.f), 15.f);
    const int iz = (int)__builtin_fminf(__builtin_fmaxf((z - lo[2]) * invh, 0.f), 15.f);
    return cs_spread4(ix) | (cs_spread4(iy) << 1) | (cs_spread4(iz) << 2);
  };
  for (int k = t; k < cnt; k += kCsThreads)
    atomicAdd(&s_cnt[cell_of(in[k * 3 + 0], in[k * 3 + 1], in[k * 3 + 2])], 1);
  __syncthreads();
  {  // exclusive prefix sum over the cells, 4 per thread; the counters then restart as the cells' fill cursors
    int v[4], sum = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[i] = s_cnt[4 * t + i];
      sum += v[i];
    }
    int base = block_exclusive_sum(sum, s_wsum);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      s_start[4 * t + i] = base;
      base += v[i];
    }
    __syncthreads();
    for (int c = t; c < kCsCells; c += kCsThreads) s_cnt[c] = 0;
    __syncthreads();
  }
  for (int k = t; k < cnt; k += kCsThreads) {
    const float x = in[k * 3 + 0], y = in[k * 3 + 1], z = in[k * 3 + 2];
    const int c = cell_of(x, y, z);
    out[s_start[c] + atomicAdd(&s_cnt[c], 1)] = make_float4(x, y, z, __int_as_float(k));
  }
  for (int k = cnt + t; k < cp; k += kCsThreads) out[k] = pad;
}

// The boxes of a side whose cp entries the workgroup has just written: tiles from the points, batches from the tiles
// (each pass reads what other threads stored: the stores are drained before the barrier).
__device__ __forceinline__ void cs_write_boxes(const CsSide &out, int cp) {
  const int t = threadIdx.x;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int tl = t; tl < cp / kCsTile; tl += kCsThreads) {
    float bl[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float bh[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    for (int i = 0; i < kCsTile; ++i) {
      const float4 p = out.pts[tl * kCsTile + i];
      if (__float_as_int(p.w) != kCsPad) {
        bl[0] = __builtin_fminf(bl[0], p.x); bh[0] = __builtin_fmaxf(bh[0], p.x);
        bl[1] = __builtin_fminf(bl[1], p.y); bh[1] = __builtin_fmaxf(bh[1], p.y);
        bl[2] = __builtin_fminf(bl[2], p.z); bh[2] = __builtin_fmaxf(bh[2], p.z);
      }
    }
    out.tbox[2 * tl + 0] = make_float4(bl[0], bl[1], bl[2], 0.f);
    out.tbox[2 * tl + 1] = make_float4(bh[0], bh[1], bh[2], 0.f);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int bt = t; bt < cp / kCsBatch; bt += kCsThreads) {
    float bl[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float bh[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    for (int i = 0; i < kCsBatch / kCsTile; ++i) {
      const float4 l = out.tbox[2 * (bt * (kCsBatch / kCsTile) + i) + 0];
      const float4 h = out.tbox[2 * (bt * (kCsBatch / kCsTile) + i) + 1];
      bl[0] = __builtin_fminf(bl[0], l.x); bh[0] = __builtin_fmaxf(bh[0], h.x);
      bl[1] = __builtin_fminf(bl[1], l.y); bh[1] = __builtin_fmaxf(bh[1], h.y);
      bl[2] = __builtin_fminf(bl[2], l.z); bh[2] = __builtin_fmaxf(bh[2], h.z);
    }
    out.bbox[2 * bt + 0] = make_float4(bl[0], bl[1], bl[2], 0.f);
    out.bbox[2 * bt + 1] = make_float4(bh[0], bh[1], bh[2], 0.f);
  }
}

// grid (2 sides, clouds)
__global__ __launch_bounds__(kCsThreads) void cs_sort_sides_kernel(
    int n1, int n2, const float *__restrict__ xyz1, const float *__restrict__ xyz2,
    char *__restrict__ scratch) {
  const int side = blockIdx.x, cloud = blockIdx.y;
  const int cnt = side == 0 ? n1 : n2;
  const long long per_cloud = cs_side_bytes(n1) + cs_side_bytes(n2);
  const CsSide out = cs_carve(scratch + (size_t)cloud * per_cloud + (side ? cs_side_bytes(n1) : 0), cnt);
  const int cp = (int)cs_round_up(cnt);
  const float inf = __builtin_inff();
  cs_sort_points((side == 0 ? xyz1 : xyz2) + (size_t)cloud * cnt * 3, cnt, out.pts, cp,
                 make_float4(inf, inf, inf, __int_as_float(kCsPad)));
  cs_write_boxes(out, cp);
}

// grid (clouds)
__global__ __launch_bounds__(kCsThreads) void cs_sort_points_kernel(int n, int npad, const float *__restrict__ xyz,
                                                                   float4 *__restrict__ sorted) {
  const int cloud = blockIdx.x;
  cs_sort_points(xyz + (size_t)cloud * n * 3, n, sorted + (size_t)cloud * npad, npad,
                 make_float4(0.f, 0.f, 0.f, __int_as_float(-1)));
}

void cs_sort_launch(int b, int n1, int n2, const float *xyz1, const float *xyz2, char *scratch, hipStream_t stream) {
  hipLaunchKernelGGL(cs_sort_sides_kernel, dim3(2, b), dim3(kCsThreads), 0, stream, n1, n2, xyz1, xyz2, scratch);
}

void cs_sort_points_launch(int b, int n, int npad, const float *xyz, float4 *sorted, hipStream_t stream) {
  hipLaunchKernelGGL(cs_sort_points_kernel, dim3(b), dim3(kCsThreads), 0, stream, n, npad, xyz, sorted);
}

}  // namespace mvp
