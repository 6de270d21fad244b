// Multi-head attention of DCP's transformer (registration/models/dcp.py: MultiHeadedAttention) in inference, as ONE kernel:
// per (cloud, head, query row i)
//   s_ij = scale * <q_i, k_j>,      out_i = sum_j softmax_j(s_ij) v_j
// q and out are (b, nq, h d), k and v (b, nk, h d), head t in the columns t d .. t d + d of a row: what the module's nn.Linear
// projections write and read, so no head transpose exists on this route.  The reference runs q k^T, the division, the
// softmax, the second product and a transposed copy as five steps over a (b, h, nq, nk) score tensor (dcp.py:26-33, 210-229);
// no score or weight ever reaches global memory here.
//
// Flash-style: a workgroup (4 waves) owns 128 consecutive queries of one (cloud, head), a wave 32 of them, and walks the keys
// in tiles of 32 with an online softmax (running maximum m and sum l per query).  Both products run on
// v_mfma_f32_32x32x2_f32 (float32 in, float32 accumulate: an fmaf chain, no reduced precision anywhere).
//   scores, "swapped":  S^T (32 keys x 32 queries) = K Q^T.  A = the key tile from LDS, one ds_read_b128 per four
//                       instructions (k permuted inside a group of 8 as csrc/edge_mlp.hip does: instruction j of group g takes
//                       column 8 g + j from lanes 0..31 and 8 g + 4 + j from lanes 32..63); B = the wave's queries, loaded
//                       once into d / 2 registers in the same permutation.  In the C layout a lane then holds ONE query
//                       (lane & 31) and 16 of its keys, (r & 3) + 8 (r >> 2) + 4 (lane >> 5): the row maximum is 15 in-lane
//                       operations and one exchange between the lane halves (v_permlane32_swap); the row sum stays per lane
//                       half and the halves meet once, after the last tile.
//   output:             O^T (d x 32 queries) += V^T P^T.  B = the 16 weight registers as they are -- instruction r sums over
//                       the keys (r & 3) + 8 (r >> 2) and that + 4, one per lane half, no cross-lane move; A = V[key][column]
//                       from LDS, one ds_read_b32 per instruction.
//   p_ij = exp2((s_ij - m) log2 e) (v_exp_f32); when the maximum moves, l and O are multiplied by exp2((m_old - m) log2 e).
//   The multiplication is skipped where that factor is exactly 1 in every lane (the same bits).  Keys past nk get the
//   score -inf (weight exactly 0) and zero rows of V; the maximum masks nothing else, so a NaN score stays a NaN weight:
//   a NaN in query i makes out_i NaN and no other row, a NaN in key j or value j every row of the (cloud, head).
//   out = O / l, IEEE division.
// Tiles.  K and V tiles of 32 keys are staged through registers into LDS, [key][d + 4] floats, double buffered: the loads of
// tile t + 1 are issued before tile t's products and written between them, one barrier per tile.  LDS: 2 buffers x 2 tensors
// x 32 x (d + 4) x 4 bytes = 67,584 (d = 128), 51,200 (96), 34,816 (64), 18,432 (32): two workgroups per CU at every d.
// Bank conflicts of that layout, from the bank maps of the three instructions: 0.  ds_read_b128 of K serves 16 lanes a
// cycle, bank (a / 4) mod 64; a lane's row starts at 4 (key (d / 4 + 1) mod 16), d / 4 + 1 is odd for d = 32, 64, 96, 128, and
// every lane group holds 16 keys distinct mod 16: 64 distinct banks.  ds_read_b32 of V: 32 consecutive floats of one row.
// ds_write_b128: 8 lanes write 32 consecutive floats of one row.
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), no spill, no scratch at any d:
//   d = 128: 224 VGPRs (0 AGPRs), 2 waves per SIMD -- what the LDS allows as well (two workgroups of four waves per CU)
//   d =  96: 176 VGPRs, 2 waves per SIMD;   d = 64: 128 VGPRs, 4 waves per SIMD;   d = 32: 78 VGPRs, 6 waves per SIMD
// (d / 2 registers hold the queries, d / 2 the output block, 16 the scores, d / 4 the next tile on its way to LDS.)
// Measured at cfg 5's shape (128, 4, 1024, 1024, 128): 2.13 ms = 129 TFLOP/s, 82 % of the 157.3 TFLOP/s float32 MFMA peak
// (profiles/dcp_attention.txt); the second wave of a SIMD runs its softmax under the first one's matrix instructions.
// Workgroups are numbered so that the query blocks of one (cloud, head) run on ONE XCD one after another (its L2 holds that
// head's keys and values for all of them), as csrc/edge_mlp.hip deals its tiles.
// No scratch memory, no atomics: every output is a fixed expression, the same bits on every run; a lane owns a query, so a
// row's bits do not depend on which other rows are in the call.
#include "common.h"

namespace mvp {

typedef float at_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kAtThreads = 256;
constexpr int kAtWaveRows = 32;                    // queries of a wave: one MFMA column block
constexpr int kAtRows = kAtThreads / 64 * kAtWaveRows;   // queries of a workgroup
constexpr int kAtKeys = 32;                        // keys of a tile
constexpr int kAtPad = 4;                          // floats; keeps rows 16-byte aligned and shifts their banks
constexpr float kAtLog2e = 1.44269504088896340736f;

constexpr int at_lds_bytes(int d) { return 2 * 2 * kAtKeys * (d + kAtPad) * 4; }

// the value of the other lane half joined with this one's: both halves get op(lower half's, upper half's)
__device__ __forceinline__ void at_halves(float x, float &lo, float &hi) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  lo = __uint_as_float(r[0]);
  hi = __uint_as_float(r[1]);
}

template <int D>
__global__ __launch_bounds__(kAtThreads, 2) void attention_forward_kernel(int h, int nq, int nk, int qblocks, long long total,
                                                                          const float *__restrict__ q,
                                                                          const float *__restrict__ k,
                                                                          const float *__restrict__ v, float scale,
                                                                          float *__restrict__ out) {
  constexpr int LD = D + kAtPad, TILE = kAtKeys * LD;          // floats of a row and of one tensor's tile in LDS
  constexpr int F4 = D / 4, PER = kAtKeys * F4 / kAtThreads;   // 16-byte pieces of a row; pieces of a tile per thread
  constexpr int CT = D / 32, G = D / 8;                        // output column blocks; groups of 8 columns
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float *lds = reinterpret_cast<float *>(smem);                // [buffer][K, V][key][LD]
  const int t = threadIdx.x, lane = t & 63, lrow = lane & 31, lk = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  // XCD x takes the work items [x per, (x + 1) per) in order: the query blocks of a (cloud, head) share an L2
  const long long per = (total + 7) / 8;
  const long long work = (long long)(blockIdx.x & 7) * per + (blockIdx.x >> 3);
  if (work >= total) return;
  const int qb = (int)(work % qblocks);
  const long long ch = work / qblocks;
  const int head = (int)(ch % h);
  const size_t cloud = (size_t)(ch / h), row = (size_t)h * D;
  const float *qc = q + cloud * nq * row + (size_t)head * D;
  const float *kc = k + cloud * nk * row + (size_t)head * D;
  const float *vc = v + cloud * nk * row + (size_t)head * D;
  float *oc = out + cloud * nq * row + (size_t)head * D;

  const int q0 = qb * kAtRows + wave * kAtWaveRows;            // the wave's first query
  const bool wave_live = q0 < nq;                              // a wave without queries only stages tiles
  const int qi = q0 + lrow;
  const bool qlive = qi < nq;                                  // an absent query computes on zeros and stores nothing

  float4 qf[G];
#pragma unroll
  for (int g = 0; g < G; ++g)
    qf[g] = qlive ? *reinterpret_cast<const float4 *>(qc + (size_t)qi * row + 8 * g + 4 * lk) : make_float4(0.f, 0.f, 0.f, 0.f);

  float4 kr[PER], vr[PER];
  auto load = [&](int j0) {                                    // tile j0 .. j0 + 32 into registers, zeros past nk
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int f = t + kAtThreads * i, key = f / F4, c4 = f - key * F4;
      const bool live = j0 + key < nk;
      const size_t at = (size_t)(j0 + key) * row + 4 * c4;
      kr[i] = live ? *reinterpret_cast<const float4 *>(kc + at) : make_float4(0.f, 0.f, 0.f, 0.f);
      vr[i] = live ? *reinterpret_cast<const float4 *>(vc + at) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto store = [&](int buf) {
    float *ks = lds + buf * 2 * TILE;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int f = t + kAtThreads * i, key = f / F4, c4 = f - key * F4;
      *reinterpret_cast<float4 *>(ks + key * LD + 4 * c4) = kr[i];
      *reinterpret_cast<float4 *>(ks + TILE + key * LD + 4 * c4) = vr[i];
    }
  };

  float m = -__builtin_inff(), l = 0.f;                        // running maximum; this lane half's share of the running sum
  at_f32x16 o[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[ct][r] = 0.f;

  const int tiles = (nk + kAtKeys - 1) / kAtKeys;
  load(0);
  store(0);
  __syncthreads();
  for (int tile = 0; tile < tiles; ++tile) {
    const bool more = tile + 1 < tiles;
    if (more) load((tile + 1) * kAtKeys);                      // in flight under this tile's scores
    const float *ks = lds + (tile & 1) * 2 * TILE, *vs = ks + TILE;
    at_f32x16 s;
    if (wave_live) {
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = 0.f;
      const float *kp = ks + lrow * LD + 4 * lk;
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float4 kf = *reinterpret_cast<const float4 *>(kp + 8 * g);
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.x, qf[g].x, s, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.y, qf[g].y, s, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.z, qf[g].z, s, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.w, qf[g].w, s, 0, 0, 0);
      }
      // register r: key tile * 32 + (r & 3) + 8 (r >> 2) + 4 lk of query qi
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] *= scale;
      if ((tile + 1) * kAtKeys > nk) {                         // the last, partial tile: the keys that do not exist
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (tile * kAtKeys + (r & 3) + 8 * (r >> 2) + 4 * lk >= nk) s[r] = -__builtin_inff();
      }
      float mx = s[0];
#pragma unroll
      for (int r = 1; r < 16; ++r) mx = __builtin_fmaxf(mx, s[r]);
      float lo, hi;
      at_halves(mx, lo, hi);
      const float mn = __builtin_fmaxf(m, __builtin_fmaxf(lo, hi));
      const float alpha = __builtin_amdgcn_exp2f((m - mn) * kAtLog2e);
      float ps = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s[r] = __builtin_amdgcn_exp2f((s[r] - mn) * kAtLog2e);
        ps += s[r];
      }
      l = __builtin_fmaf(l, alpha, ps);
      m = mn;
      if (__builtin_amdgcn_ballot_w64(alpha != 1.f) != 0) {    // times exactly 1 otherwise: the same bits
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[ct][r] *= alpha;
      }
    }
    if (more) store((tile + 1) & 1);                           // last read before the previous barrier
    if (wave_live) {
      const float *vp = vs + 4 * lk * LD + lrow;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = (r & 3) + 8 * (r >> 2);
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
          o[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[key * LD + 32 * ct], s[r], o[ct], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  if (!wave_live) return;
  float lo, hi;
  at_halves(l, lo, hi);
  l = lo + hi;
  if (!qlive) return;
  // register 4 rg + i of block ct: column 32 ct + 8 rg + 4 lk + i of this lane's query
  float *op = oc + (size_t)qi * row + 4 * lk;
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int rg = 0; rg < 4; ++rg)
      *reinterpret_cast<float4 *>(op + 32 * ct + 8 * rg) =
          make_float4(o[ct][4 * rg] / l, o[ct][4 * rg + 1] / l, o[ct][4 * rg + 2] / l, o[ct][4 * rg + 3] / l);
}

template <int D>
static int at_launch(int b, int h, int nq, int nk, const float *q, const float *k, const float *v, float scale, float *out,
                     void *stream) {
  static_assert(D % 32 == 0 && kAtKeys * (D / 4) % kAtThreads == 0 && 2 * at_lds_bytes(D) <= 160 * 1024, "tile");
  const auto kernel = attention_forward_kernel<D>;
  if (hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          at_lds_bytes(D)) != hipSuccess)
    return check_launch("mvp_attention_forward");
  const int qblocks = (nq + kAtRows - 1) / kAtRows;
  const long long total = (long long)b * h * qblocks;
  const dim3 grid((unsigned)((total + 7) / 8 * 8));
  hipLaunchKernelGGL(kernel, grid, dim3(kAtThreads), at_lds_bytes(D), as_stream(stream), h, nq, nk, qblocks, total, q, k, v,
                     scale, out);
  return check_launch("mvp_attention_forward");
}

}  // namespace mvp

using namespace mvp;

extern "C" int mvp_attention_forward(int b, int h, int nq, int nk, int d, const float *q, const float *k, const float *v,
                                     float scale, float *out, void *stream) {
  if (b < 0 || h < 1 || nq < 0 || nk < 0 || !(d == 32 || d == 64 || d == 96 || d == 128)) return MVP_EBADARG;
  if (b == 0 || nq == 0) return MVP_OK;
  if (nk == 0) return MVP_EBADARG;
  const long long row = (long long)h * d, most = 2147483647LL;
  if (row > most || (long long)b * nq > most / row || (long long)b * nk > most / row) return MVP_EBADARG;   // 2^31 elements
  if (!q || !k || !v || !out || misaligned(q) || misaligned(k) || misaligned(v) || misaligned(out)) return MVP_EBADARG;
  switch (d) {
    case 32: return at_launch<32>(b, h, nq, nk, q, k, v, scale, out, stream);
    case 64: return at_launch<64>(b, h, nq, nk, q, k, v, scale, out, stream);
    case 96: return at_launch<96>(b, h, nq, nk, q, k, v, scale, out, stream);
    default: return at_launch<128>(b, h, nq, nk, q, k, v, scale, out, stream);
  }
}
