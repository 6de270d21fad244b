// DGCNN's edge MLP (registration/models/dcp.py: DGCNN) in inference: the k-neighbourhood gather, up to four 1x1 convolutions
// with a per-channel affine map (BatchNorm in eval mode) and ReLU, and the max over the k neighbours after each, as ONE
// kernel.  Per cloud, point p, slot j:
//   e_0[:, j] = [x[:, idx[j, p]] ; x[:, p]]                       (neighbour first, then centre: get_graph_feature's order)
//   e_i[:, j] = relu(scale_i * (W_i e_{i-1}[:, j]) + shift_i)     i = 1 .. stages      relu(t) = t < 0 ? 0 : t
//   out[off_i : off_i + w_i, p] = max_j e_i[:, j]                 NaN if a member is (torch.max)
// The reference has no kernel for it (registration/models/dcp.py:286-318 runs conv / BatchNorm / ReLU / max op by op on
// (B, C, N, k) tensors); no (b, C, k, n) tensor exists in global memory here.
//
// Tile.  A workgroup (4 waves) owns `pts` consecutive points of one cloud: pts * k <= cols = 32 * ncb columns, ncb = 2 (1
// where a whole cloud fits 32 columns); column j * pts + p is slot j of the tile's point p (so idx, k-major, is read in
// runs along n), the columns past pts * k and the points past n are computed on zeros and never reach a maximum.  The
// activations live in LDS as [channel][column] float rows of cols + 4 floats: stage i reads its input region and writes
// its output region, the two regions alternate between the bottom and the top of one image of `rows` rows, rows = the
// largest (input + output) of any stage; the LAST stage's output is only reduced, so it goes through a chunk of at most
// 128 rows.  DGCNN (64, 64, 128, 256; k = 20): 3 points a tile (60 of 64 columns), 256 + 8 rows x 68 floats = 71,808
// bytes of the 160 KiB -- two workgroups per CU, so one's gather, stage 1, maxima and barriers run under the other's
// matrix instructions.  (Measured at cfg 5, 256 clouds x 1024 points, the kernel alone: 128-column tiles, one workgroup
// per CU, 8.09 ms; 64-column tiles 6.80 ms, although every tile streams the weights and the weights' L2 traffic doubles.)
// Workgroups are numbered so that the tiles of one cloud run on ONE XCD one after another (its L2 holds the cloud's points
// and joins the short runs neighbouring tiles write into a row of `out`).
//
// Stage 1 (K = 2c <= 8) is VALU work on the gathered values (an 8-row image of their own), an fmaf chain over ascending
// input channels.  Stages 2..4 run on v_mfma_f32_32x32x2_f32 (float32 in, float32 accumulate): a wave takes a block of 32
// output channels x tn * 32 columns (tn = ncb, or a share of the columns where a round has fewer than four channel
// blocks: one unit per wave), the B operand is one ds_read_b32 per instruction from the input region, the A operand -- the weights, (w_i,
// w_{i-1}) row-major -- streams from global memory / L2 in 16-byte reads of a row (k permuted inside a group of 8 the
// way csrc/pointwise_mfma.hip does: instruction j takes k = j from lanes 0..31 and k = 4 + j from lanes 32..63), a
// slab of 32 values of k ahead of the matrix instructions that use it; the B fragments are read a group of 8 values of k
// ahead (em_block).  The K loop of pointwise_k_loop.inc is not used: it
// stages BOTH operands from global memory through double-buffered LDS slabs, here B already lies in LDS whole and A
// needs no LDS at all.
// After a round of at most 128 output channels: one barrier, then every thread takes (channel, point) pairs and walks the
// k columns of its point; the next round's or stage's matrix work needs no second barrier (it reads what the maxima
// read and writes elsewhere), only the last stage's chunk is reused and waits.
// No scratch memory, no atomics: every output is a fixed expression, the same bits on every run.
#include "common.h"

namespace mvp {

typedef float em_f32x16 __attribute__((ext_vector_type(16)));

constexpr int kEmThreads = 256;
constexpr int kEmPad = 4;            // floats; keeps rows 16-byte aligned and shifts their banks
constexpr int kEmChunk = 128;        // output channels per round: 4 waves x 32
constexpr int kEmGatherRows = 8;     // 2c <= 8 gathered rows
constexpr int kEmMaxNcb = 2;         // 32-column blocks of the widest tile
constexpr int kEmLaneCols = kEmMaxNcb * 32 / 64;   // columns of a tile per lane of a wave
constexpr int kEmLdsMax = 160 * 1024;
constexpr int kEmMaxStages = 4, kEmMaxWidth = 256, kEmMaxC = 4, kEmMaxK = 64;

struct EmPlan {
  int c, n, k, stages;
  int w[kEmMaxStages];
  int ncb;      // 32-column blocks of a tile
  int pts;      // points of a tile: 32 * ncb / k
  int rows;     // rows of the activation image
  int b, tiles; // clouds, tiles of a cloud
};

__host__ __device__ inline int em_out_rows(const EmPlan &pl, int st) {     // rows of stage st's output region
  return st == pl.stages - 1 && pl.w[st] > kEmChunk ? kEmChunk : pl.w[st];
}

__device__ __forceinline__ float em_relu(float v) { return v < 0.f ? 0.f : v; }

// The B fragments of one group of 8 values of k: b[j][i] is instruction j's operand for column block i
template <int TN>
__device__ __forceinline__ void em_frag(float (&b)[4][TN], const float *bp, int ld) {
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < TN; ++i) b[j][i] = bp[j * ld + i * 32];
}

// One block of 32 output channels x TN * 32 columns: acc = W[32 rows][K] x in[K][columns], then the affine map and ReLU,
// written to `outp`.  wl: this lane's weight row at its k offset (row lrow, + 4 lk); bl: the input region at this lane's
// column (+ 4 lk rows); outp: the output region at the block's first row and this lane's column; sc / sh: the block's
// first row of scale / shift.
// The fragments of group kg + 1 are read from LDS, and the weights of slab s + 1 from memory, BEFORE the matrix
// instructions of group kg are issued, and the scheduler is kept from moving them back down (left to itself it issues each
// ds_read right in front of the two instructions that use it and waits for it there: 2 instructions per LDS round trip).
template <int TN>
__device__ __forceinline__ void em_block(const float *__restrict__ wl, int K, const float *bl, int ld, float *outp,
                                         const float *__restrict__ sc, const float *__restrict__ sh, int lk) {
  em_f32x16 acc[TN];
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  float4 cur[4], nxt[4];
  float b[2][4][TN];
  float fa[16], fb[16];                                      // the rows' scale and shift: asked for now, used at the end
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    fa[r] = sc[(r & 3) + 8 * (r >> 2) + 4 * lk];
    fb[r] = sh[(r & 3) + 8 * (r >> 2) + 4 * lk];
  }
#pragma unroll
  for (int kg = 0; kg < 4; ++kg) cur[kg] = *reinterpret_cast<const float4 *>(wl + kg * 8);
  em_frag<TN>(b[0], bl, ld);
  for (int s = 0; s < K; s += 32) {
    const bool more = s + 32 < K;
    if (more) {                                              // in flight while this slab computes
#pragma unroll
      for (int kg = 0; kg < 4; ++kg) nxt[kg] = *reinterpret_cast<const float4 *>(wl + s + 32 + kg * 8);
    }
#pragma unroll
    for (int kg = 0; kg < 4; ++kg) {
      if (kg < 3 || more) em_frag<TN>(b[(kg + 1) & 1], bl + (s + (kg + 1) * 8) * ld, ld);
      __builtin_amdgcn_sched_barrier(0);
      const float av[4] = {cur[kg].x, cur[kg].y, cur[kg].z, cur[kg].w};
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < TN; ++i)
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], b[kg & 1][j][i], acc[i], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (more) {
#pragma unroll
      for (int kg = 0; kg < 4; ++kg) cur[kg] = nxt[kg];
    }
  }
  // C/D layout: register r of a lane holds column lane & 31 and row (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of the block
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * lk;
#pragma unroll
    for (int i = 0; i < TN; ++i) outp[row * ld + i * 32] = em_relu(__builtin_fmaf(fa[r], acc[i][r], fb[r]));
  }
}

// Stage 1 of one round (rows r0 .. r0 + nr of W_1, (w_1, 2C) row-major): a wave takes 16 channels at a time -- their weights,
// scale and shift are uniform, so they come through scalar loads, 2C of them in one piece (C is a template parameter for
// that: with a run-time row length every weight was a guarded load and a wait of its own) -- and a lane its columns, whose
// gathered values it holds in ev.
template <int C>
__device__ __forceinline__ void em_stage1(const float *__restrict__ w1, const float *__restrict__ sc,
                                          const float *__restrict__ sh, int r0, int nr,
                                          const float (&ev)[kEmLaneCols][kEmGatherRows], float *outr, int ld, int cols,
                                          int lane, int wave) {
  for (int g = wave; g < nr / 16; g += kEmThreads / 64) {
#pragma unroll 4
    for (int ch = 0; ch < 16; ++ch) {
      const int row = r0 + g * 16 + ch;
      float wv[2 * C];
#pragma unroll
      for (int kk = 0; kk < 2 * C; ++kk) wv[kk] = w1[row * 2 * C + kk];
      const float fa = sc[row], fb = sh[row];
#pragma unroll
      for (int ci = 0; ci < kEmLaneCols; ++ci) {
        float acc = 0.f;
#pragma unroll
        for (int kk = 0; kk < 2 * C; ++kk) acc = __builtin_fmaf(wv[kk], ev[ci][kk], acc);
        if (lane + 64 * ci < cols) outr[(g * 16 + ch) * ld + lane + 64 * ci] = em_relu(__builtin_fmaf(fa, acc, fb));
      }
    }
  }
}

__global__ __launch_bounds__(kEmThreads) void edge_mlp_max_kernel(EmPlan pl, const float *__restrict__ x,
                                                                  const int *__restrict__ idx,
                                                                  const float *__restrict__ w,
                                                                  const float *__restrict__ scale,
                                                                  const float *__restrict__ shift,
                                                                  float *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float *img = reinterpret_cast<float *>(smem);
  const int t = threadIdx.x, lane = t & 63, lrow = lane & 31, lk = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);   // uniform, and known to be
  const int n = pl.n, k = pl.k, c = pl.c, pts = pl.pts, ncb = pl.ncb;
  const int cols = 32 * ncb, ld = cols + kEmPad;
  // Workgroups are dealt to the 8 XCDs round-robin by their number: XCD x takes the tiles [x per, (x + 1) per) in order, so
  // the tiles of a cloud run on ONE XCD one after another -- the cloud's points stay in its L2, and the 4 * pts-byte pieces
  // that neighbouring tiles write into one row of `out` meet there before the row leaves for memory.
  const long long total = (long long)pl.tiles * pl.b, per = (total + 7) / 8;
  const long long work = (long long)(blockIdx.x & 7) * per + (blockIdx.x >> 3);
  if (work >= total) return;
  const int cloud = (int)(work / pl.tiles), p0 = (int)(work % pl.tiles) * pts;
  const int np = min(pts, n - p0);                           // this tile's points that exist (>= 1)
  const size_t ns = (size_t)n;
  int sumw = 0;
  for (int st = 0; st < pl.stages; ++st) sumw += pl.w[st];
  const float *xc = x + (size_t)cloud * c * ns;
  const int *ic = idx + (size_t)cloud * k * ns;
  float *oc = out + (size_t)cloud * sumw * ns;

  // ---- the gathered values [neighbour ; centre], zeros in the columns nobody owns
  float *e0 = img + pl.rows * ld;
  for (int col = t; col < cols; col += kEmThreads) {
    const int j = col / pts, p = col - j * pts;
    const bool live = j < k && p < np;
    int src = 0;
    if (live) src = min(max(ic[(size_t)j * ns + p0 + p], 0), n - 1);
#pragma unroll
    for (int ch = 0; ch < kEmMaxC; ++ch) {
      if (ch < c) {
        e0[ch * ld + col] = live ? xc[(size_t)ch * ns + src] : 0.f;
        e0[(c + ch) * ld + col] = live ? xc[(size_t)ch * ns + p0 + p] : 0.f;
      }
    }
  }
  __syncthreads();

  float ev[kEmLaneCols][kEmGatherRows];                      // this lane's columns of it, for stage 1
#pragma unroll
  for (int ci = 0; ci < kEmLaneCols; ++ci)
#pragma unroll
    for (int kk = 0; kk < kEmGatherRows; ++kk)
      ev[ci][kk] = (kk < 2 * c && lane + 64 * ci < cols) ? e0[kk * ld + lane + 64 * ci] : 0.f;

  // the maxima's (channel, point) pairs: thread t takes point t % pts of channels t / pts, t / pts + 256 / pts, ..
  const int mi = t / pts, mp = mi < kEmThreads / pts ? t - mi * pts : pts;

  const float *in = e0;
  const float *wst = w;                                      // this stage's weights, scale / shift and output rows
  int off = 0;
  for (int st = 0; st < pl.stages; ++st) {
    const int K = st == 0 ? 2 * c : pl.w[st - 1], wd = pl.w[st];
    const bool last = st == pl.stages - 1;
    float *outb = img + ((st & 1) ? pl.rows - em_out_rows(pl, st) : 0) * ld;
    const float *sc = scale + off, *sh = shift + off;
    for (int r0 = 0; r0 < wd; r0 += kEmChunk) {
      const int nr = min(kEmChunk, wd - r0);
      float *outr = outb + (last ? 0 : r0) * ld;            // the round's first row in LDS
      if (st == 0) {
        switch (c) {
          case 1: em_stage1<1>(wst, sc, sh, r0, nr, ev, outr, ld, cols, lane, wave); break;
          case 2: em_stage1<2>(wst, sc, sh, r0, nr, ev, outr, ld, cols, lane, wave); break;
          case 3: em_stage1<3>(wst, sc, sh, r0, nr, ev, outr, ld, cols, lane, wave); break;
          default: em_stage1<4>(wst, sc, sh, r0, nr, ev, outr, ld, cols, lane, wave); break;
        }
      } else {
        // rbn blocks of 32 channels; with fewer than four the columns are shared out too: one unit per wave
        const int rbn = nr / 32;
        const int cg = rbn >= 3 ? 1 : min(ncb, 4 / rbn);
        const int tn = ncb / cg;
        if (wave < rbn * cg) {
          const int rb = wave / cg, col0 = (wave % cg) * tn * 32;
          const int row0 = r0 + rb * 32;
          const float *wl = wst + (size_t)(row0 + lrow) * K + 4 * lk;
          const float *bl = in + 4 * lk * ld + col0 + lrow;
          float *outp = outr + rb * 32 * ld + col0 + lrow;
          if (tn == 2) em_block<2>(wl, K, bl, ld, outp, sc + row0, sh + row0, lk);
          else em_block<1>(wl, K, bl, ld, outp, sc + row0, sh + row0, lk);
        }
      }
      __syncthreads();
      // the maxima of this round's rows: a thread per (channel, point), the k slots pts columns apart, eight reads in
      // flight at a time (a slot past k counts as slot k - 1 again; one read per trip is one LDS latency per slot)
      if (mp < np) {
        for (int i = mi; i < nr; i += kEmThreads / pts) {
          const float *src = outr + i * ld + mp;
          float m = src[0];
          for (int j0 = 0; j0 < k; j0 += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = src[min(j0 + u, k - 1) * pts];
#pragma unroll
            for (int u = 0; u < 8; ++u) m = (v[u] > m || v[u] != v[u]) ? v[u] : m;      // a NaN member stays (torch.max)
          }
          oc[(size_t)(off + r0 + i) * ns + p0 + mp] = m;
        }
      }
      if (last && r0 + kEmChunk < wd) __syncthreads();      // the chunk is written again
    }
    in = outb;
    wst += (size_t)wd * K;
    off += wd;
  }
}

// The shapes the entry point takes, and the plan of a covered one.
static bool em_plan(int b, int c, int n, int k, int stages, const int (&w)[kEmMaxStages], EmPlan &pl) {
  if (b < 0 || n < 0 || b > 65535 || c < 1 || c > kEmMaxC || k < 1 || k > kEmMaxK || stages < 1 || stages > kEmMaxStages)
    return false;
  for (int st = 0; st < kEmMaxStages; ++st) {
    if (st < stages ? (w[st] < 32 || w[st] > kEmMaxWidth || (w[st] & 31) != 0) : w[st] != 0) return false;
  }
  if ((long long)n * k > 2147483647LL) return false;       // a cloud's index slab is counted in an int by the callers
  pl.c = c, pl.n = n, pl.k = k, pl.stages = stages;
  for (int st = 0; st < kEmMaxStages; ++st) pl.w[st] = w[st];
  pl.rows = 0;
  for (int st = 0; st < stages; ++st) {
    const int need = (st == 0 ? 0 : w[st - 1]) + em_out_rows(pl, st);
    pl.rows = need > pl.rows ? need : pl.rows;
  }
  // the widest tile (its image fits whatever the widths: 512 + 8 rows of 68 floats), narrower where the whole cloud fits half
  static_assert((2 * kEmMaxWidth + kEmGatherRows) * (32 * kEmMaxNcb + kEmPad) * 4 <= kEmLdsMax && 32 * kEmMaxNcb >= kEmMaxK,
                "every covered shape has a tile");
  pl.ncb = kEmMaxNcb;
  while (pl.ncb > 1 && k <= 16 * pl.ncb && (long long)n * k <= 16 * pl.ncb) pl.ncb >>= 1;
  pl.pts = 32 * pl.ncb / k;
  pl.b = b;
  pl.tiles = (n + pl.pts - 1) / pl.pts;
  return (long long)pl.tiles * b <= 2147483640LL;            // the grid: one workgroup per tile, rounded up to the 8 XCDs
}

}  // namespace mvp

using namespace mvp;

extern "C" int mvp_edge_mlp_max(int b, int c, int n, int k, int stages, int w1, int w2, int w3, int w4, const float *x,
                                const int *idx, const float *w, const float *scale, const float *shift, float *out,
                                void *stream) {
  const int widths[kEmMaxStages] = {w1, w2, w3, w4};
  EmPlan pl;
  if (!em_plan(b, c, n, k, stages, widths, pl)) return MVP_EBADSHAPE;
  if (b == 0 || n == 0) return MVP_OK;
  if (!x || !idx || !w || !scale || !shift || !out) return MVP_EBADARG;
  if (misaligned(w)) return MVP_EBADARG;      // the weights' rows are read 16 bytes at a time
  const int lds = (pl.rows + kEmGatherRows) * (32 * pl.ncb + kEmPad) * 4;
  if (hipFuncSetAttribute(reinterpret_cast<const void *>(edge_mlp_max_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          lds) != hipSuccess)
    return check_launch("mvp_edge_mlp_max");
  const dim3 grid((unsigned)(((long long)pl.tiles * b + 7) / 8 * 8));
  hipLaunchKernelGGL(edge_mlp_max_kernel, grid, dim3(kEmThreads), lds, as_stream(stream), pl, x, idx, w, scale, shift, out);
  return check_launch("mvp_edge_mlp_max");
}
