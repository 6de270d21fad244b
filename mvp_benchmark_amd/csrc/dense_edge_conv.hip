// Dense edge convolution of ECG (completion/models/edge_unet.py: Dense_conv), forward and backward, with everything
// that is per EDGE kept in registers.  L = dense_n - 1 stack layers, growth rate G, k neighbours:
//   edge[:, j]  = relu(a[:, n] + nb[idx[j, n], :])
//   y_i[:, j]   = act_i(W_i [edge; y_1; ..; y_{i-1}][:, j] + ctr_i[:, n])     act_i = ReLU for i < L, identity for i = L
//   out[b, :, n] = [max_j edge, max_j y_1, .., max_j y_L]     arg[b, c, n] = the FIRST maximal j (mvp_gather_max's rule)
// The reference has no kernel for it (completion/models/ecg.py:36-65 runs conv / ReLU / cat / max op by op on the
// (B, ., N, k) tensors); the composed route of Dense_conv.forward materialises ~10 (B, G, k, N) tensors each way.
//
// Layouts.  a (B, G, N), ctr (B, L*G, N), out (B, (L+1)*G, N), arg likewise, idx (B, k, N) k-major: channel-major, N
// contiguous -- a lane owns one point n and loops over the k slots, so all of these are coalesced.  nb is taken
// POINT-major, (B, N, G), 16-byte aligned: a neighbour's G values are one contiguous 4G-byte read (the caller
// transposes once; a cloud's copy is <= 295 KB and stays in cache).  No scratch in the forward.  w: layer i
// (1-based) is (G, i*G) row-major over the input channels [edge, y_1 .. y_{i-1}], layers back to back.
// The weights are uniform across lanes and are read through scalar loads, streamed in chunks (de_layer).
//
// Arithmetic: y_i[c] = fma chain over the input channels in ascending order, started from ctr_i[c]; nothing depends on
// the launch geometry.  Indices are clamped into [0, N).  Behaviour on non-finite inputs is unspecified in this version
// (a NaN never becomes a maximum; the ReLU masks of the backward treat it as "not positive").
//
// Backward.  One launch recomputes edge and y_1 .. y_{L-1} per slot from the inputs, routes grad_out to the slot `arg`
// names, and walks the layers down:
//   gy_L = grad_out_L at j == arg_L, gy_i = (W_{i+1..L}^T gy + grad_out_i at arg_i) * (y_i > 0),
//   grad_edge[b, :, j, n] = the same at the pre-ReLU edge sum (the ONE (B, G, k, N) temporary; the grouping operator's
//   scatter sums it into grad_nb), grad_a = sum_j grad_edge, grad_ctr_i = sum_j gy_i (grad_ctr_L = grad_out_L).
// Weight gradient: a workgroup is ONE wave of 64 points.  Per slot the wave stages its 64 edges' input vectors
// [edge; y..] and, layer by layer, their gy_i in LDS; lane (r, q) of an 8 x 8 grid owns the (G/8) x (i*G/8) block
// of grad W_i and adds the 64 outer products in ascending lane order.  (Layer L's gy is non-zero at one slot per point
// and channel only; it takes the same dense path -- one code path for all layers, a known cost.)  The workgroup's sums
// go to its slot of the caller's scratch, B * ceil(N/64) slots; a second launch adds the slots in a fixed order (eight
// interleaved chains in ascending slot order, then the chains in ascending order): no float atomics, the same bits on
// every run.
//
// Registers (gfx950, __launch_bounds__(256), launched with 64 threads; vgpr_count of the code-object notes, AGPRs
// included; every kernel: private_segment_fixed_size 0, no vector-register spill -- no scratch memory):
//   forward   G  8: L0 30, L1 55,  L2 69  | G 16: 60, 112, 135 | G 24: 90, 169, 205  | G 32: 115, 219, 252
//   backward  G  8: L0 41, L1 70,  L2 115 | G 16: 72, 138, 231 | G 24: 131, 216, 356 | G 32: 162, 282, 466
//   (above 256 the kernel runs one wave per SIMD; ECG's shape is G 24, L 2)   second pass of grad_w: 10
#include "common.h"

namespace mvp {

constexpr int kDeThreads = 64;     // one wave: a lane per point
constexpr int kDeMaxK = 64;
constexpr int kDeMaxN = 65536;   // g * k * n * 4 bytes, the largest slab of a cloud, stays below 2^31

__host__ __device__ constexpr int de_w_off(int g, int i) { return g * g * ((i - 1) * i / 2); }   // first float of layer i
__host__ __device__ constexpr int de_w_floats(int g, int layers) { return de_w_off(g, layers + 1); }

static bool de_shape_ok(int b, int g, int layers, int k, int n) {
  return b >= 0 && n >= 0 && n <= kDeMaxN && b <= 65535 && (g == 8 || g == 16 || g == 24 || g == 32) && layers >= 0 && layers <= 2 &&
         k >= 1 && k <= kDeMaxK;
}

// A uniform zero the optimiser cannot see through, available only once `after` has been computed.  An address plus
// this stays a scalar address but is not invariant in the slot loop and not known before `after`: the loads through it
// stay inside the loop, behind the arithmetic that produced `after`.  (Hoisted out of the loop, or to the top of its
// body, the g*g*L(L+1)/2 weights and the rows' byte offsets would have to live in, and spill from, the scalar registers.)
__device__ __forceinline__ int de_opaque_zero(float after) {
  int z = 0;
  asm volatile("" : "+s"(z) : "v"(after));
  return z;
}

// Addressing: every per-point array of a cloud is read and written through a buffer resource of that cloud's slab, a
// row's byte offset in a scalar register and the lane's point `up` as a 32-bit byte offset -- not a 64-bit lane address
// per channel kept in vector registers (a slab is < 2^31 bytes: n <= kDeMaxN).
typedef decltype(__builtin_amdgcn_make_buffer_rsrc((void *)nullptr, (short)0, 0, 0)) DeRsrc;
__device__ __forceinline__ DeRsrc de_slab(const void *base, size_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ int de_ldi(DeRsrc rs, unsigned up, int row, int n) {
  return (int)__builtin_amdgcn_raw_buffer_load_b32(rs, up, row * n * 4, 0);
}
__device__ __forceinline__ float de_ldf(DeRsrc rs, unsigned up, int row, int n) {
  return __int_as_float(de_ldi(rs, up, row, n));
}
__device__ __forceinline__ void de_sti(DeRsrc rs, unsigned up, int row, int n, int v) {
  __builtin_amdgcn_raw_buffer_store_b32(v, rs, up, row * n * 4, 0);
}
__device__ __forceinline__ void de_stf(DeRsrc rs, unsigned up, int row, int n, float v) {
  de_sti(rs, up, row, n, __float_as_int(v));
}

// One layer's products with its (G, IG) row-major weights at `w` (uniform):
//   FORWARD   y[c]  = fma(W[c][ci], x[ci], y[c])    for ci ascending, every c      (y preset to the centre term)
//   otherwise y[ci] = fma(W[c][ci], x[c], y[ci])    for c ascending, every ci      (W^T x, added to y)
// The weights are a stream of kDeChunk-float chunks in memory order; chunk q + 1 is loaded (scalar loads) while the
// lanes multiply with chunk q, its address tied to chunk q - 1's last product (de_opaque_zero), and nothing is
// scheduled across a chunk's end -- two chunks of scalar registers at a time, however long the layer.  G * IG is a multiple of 64 for every G the kernels are built for.
constexpr int kDeChunk = 32;

template <int G, int IG, bool FORWARD>
__device__ __forceinline__ void de_layer(const float *__restrict__ w, const float *x, float *y) {
  constexpr int kChunks = G * IG / kDeChunk;
  static_assert(G * IG % kDeChunk == 0, "whole chunks");
  float cur[kDeChunk], nxt[kDeChunk];
  float tie = FORWARD ? y[0] : x[0];                // chunk q + 1 is asked for once chunk q - 1 has been used
  const float *w0 = w + de_opaque_zero(tie);
#pragma unroll
  for (int e = 0; e < kDeChunk; ++e) cur[e] = w0[e];
#pragma unroll
  for (int q = 0; q < kChunks; ++q) {
    if (q + 1 < kChunks) {
      const float *wq = w + (q + 1) * kDeChunk + de_opaque_zero(tie);
#pragma unroll
      for (int e = 0; e < kDeChunk; ++e) nxt[e] = wq[e];
    }
#pragma unroll
    for (int e = 0; e < kDeChunk; ++e) {
      const int c = (q * kDeChunk + e) / IG, ci = (q * kDeChunk + e) % IG;
      if (FORWARD) tie = y[c] = __builtin_fmaf(cur[e], x[ci], y[c]);
      else tie = y[ci] = __builtin_fmaf(cur[e], x[c], y[ci]);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int e = 0; e < kDeChunk; ++e) cur[e] = nxt[e];
  }
}

// edge = relu(a + nb row), y_i for i <= LAST (post-ReLU) into in[0 .. LAST*G + G)
template <int G, int LAST>
__device__ __forceinline__ void de_edge_stack(const float *__restrict__ row, const float (&av)[G],
                                              DeRsrc ctr_s, int n, unsigned up,
                                              const float *__restrict__ w, float *in) {
#pragma unroll
  for (int c = 0; c < G; c += 4) {
    const float4 r = *reinterpret_cast<const float4 *>(row + c);
    in[c] = fmaxf(av[c] + r.x, 0.f);
    in[c + 1] = fmaxf(av[c + 1] + r.y, 0.f);
    in[c + 2] = fmaxf(av[c + 2] + r.z, 0.f);
    in[c + 3] = fmaxf(av[c + 3] + r.w, 0.f);
  }
#pragma unroll
  for (int i = 1; i <= LAST; ++i) {
#pragma unroll
    for (int c = 0; c < G; ++c) in[i * G + c] = de_ldf(ctr_s, up, (i - 1) * G + c, n);
    if (i == 1) de_layer<G, G, true>(w, in, in + G);                 // (i is a constant once unrolled; L <= 2 keeps LAST <= 1)
#pragma unroll
    for (int c = 0; c < G; ++c) in[i * G + c] = fmaxf(in[i * G + c], 0.f);
  }
}

template <int G, int L>
__global__ __launch_bounds__(256) void dense_edge_conv_kernel(
    int k, int n, const float *__restrict__ a, const float *__restrict__ nb, const int *__restrict__ idx,
    const float *__restrict__ ctr, const float *__restrict__ w, float *__restrict__ out, int *__restrict__ arg) {
  static_assert(L <= 2, "de_edge_stack instantiates de_layer for layer 1 only");
  constexpr int C = (L + 1) * G;
  constexpr int LAST = L > 0 ? L - 1 : 0;           // layers whose output feeds another layer
  const int p = blockIdx.x * kDeThreads + threadIdx.x;
  if (p >= n) return;
  const unsigned up = 4u * (unsigned)p;
  const int cloud = blockIdx.y;
  const size_t ns = (size_t)n;
  const DeRsrc as = de_slab(a + (size_t)cloud * G * ns, G * ns * 4);
  const DeRsrc cs = de_slab(ctr + (size_t)cloud * L * G * ns, L * G * ns * 4);     // not used when L == 0
  const DeRsrc is = de_slab(idx + (size_t)cloud * k * ns, k * ns * 4);
  const float *nbc = nb + (size_t)cloud * ns * G;
  float av[G];
#pragma unroll
  for (int c = 0; c < G; ++c) av[c] = de_ldf(as, up, c, n);
  float best[C];
#pragma unroll
  for (int c = 0; c < C; ++c) best[c] = -INFINITY;
  unsigned slot[C / 4];                                          // four 8-bit slots per register (k <= 64)
#pragma unroll
  for (int c = 0; c < C / 4; ++c) slot[c] = 0u;
  for (int j = 0; j < k; ++j) {
    const int src = min(max(de_ldi(is, up, j, n), 0), n - 1);
    const int nj = n + de_opaque_zero(__int_as_float(src));      // the rows' byte offsets: computed per slot, not kept
    float in[(LAST + 1) * G];
    const float *wj = w;
    de_edge_stack<G, LAST>(nbc + (size_t)src * G, av, cs, nj, up, wj, in);
    auto take = [&](int c, float v) {
      const bool gt = v > best[c];                               // strict: the first maximal slot stays
      best[c] = gt ? v : best[c];
      const unsigned sh = 8u * (c & 3);
      slot[c >> 2] = gt ? ((slot[c >> 2] & ~(0xffu << sh)) | ((unsigned)j << sh)) : slot[c >> 2];
    };
#pragma unroll
    for (int c = 0; c < (L > 0 ? L : 1) * G; ++c) take(c, in[c]);
    if constexpr (L > 0) {
      float y[G];                                                // the last layer has no activation
#pragma unroll
      for (int c = 0; c < G; ++c) y[c] = de_ldf(cs, up, (L - 1) * G + c, nj);
      de_layer<G, L * G, true>(wj + de_w_off(G, L), in, y);
#pragma unroll
      for (int c = 0; c < G; ++c) take(L * G + c, y[c]);
    }
  }
  const DeRsrc os = de_slab(out + (size_t)cloud * C * ns, C * ns * 4);
  const DeRsrc gs = de_slab(arg + (size_t)cloud * C * ns, C * ns * 4);
#pragma unroll
  for (int c = 0; c < C; ++c) {
    de_stf(os, up, c, n, best[c]);
    de_sti(gs, up, c, n, (int)((slot[c >> 2] >> (8 * (c & 3))) & 0xffu));
  }
}

// LDS of one workgroup of the backward: 64 rows of [edge; y..] and 64 rows of one layer's gy, rows padded by one float
template <int G, int L>
struct DeStage {
  static constexpr int kIn = (L > 0 ? L : 1) * G + 1, kGy = G + 1;
};

template <int G, int L>
__global__ __launch_bounds__(256) void dense_edge_conv_grad_kernel(
    int k, int n, const float *__restrict__ a, const float *__restrict__ nb, const int *__restrict__ idx,
    const float *__restrict__ ctr, const float *__restrict__ w, const int *__restrict__ arg,
    const float *__restrict__ grad_out, float *__restrict__ grad_a, float *__restrict__ grad_edge,
    float *__restrict__ grad_ctr, float *__restrict__ partial) {
  constexpr int C = (L + 1) * G;
  constexpr int LAST = L > 0 ? L - 1 : 0;
  constexpr int T = G / 8;                          // a lane's block of grad W_i: T rows x (i * T) columns
  constexpr int kIn = DeStage<G, L>::kIn, kGy = DeStage<G, L>::kGy;
  __shared__ float s_in[L > 0 ? kDeThreads * kIn : 1];
  __shared__ float s_gy[L > 0 ? kDeThreads * kGy : 1];
  const int t = threadIdx.x;
  const int p = blockIdx.x * kDeThreads + t;
  const bool live = p < n;                          // a lane past the end stays for the barriers and stages zeros
  const unsigned up = 4u * (unsigned)(live ? p : n - 1);
  const int cloud = blockIdx.y;
  const size_t ns = (size_t)n;
  const DeRsrc as = de_slab(a + (size_t)cloud * G * ns, G * ns * 4);
  const DeRsrc cs = de_slab(ctr + (size_t)cloud * L * G * ns, L * G * ns * 4);
  const DeRsrc is = de_slab(idx + (size_t)cloud * k * ns, k * ns * 4);
  const float *nbc = nb + (size_t)cloud * ns * G;
  const DeRsrc gos = de_slab(grad_out + (size_t)cloud * C * ns, C * ns * 4);
  const DeRsrc ags = de_slab(arg + (size_t)cloud * C * ns, C * ns * 4);
  const DeRsrc ges = de_slab(grad_edge ? grad_edge + (size_t)cloud * G * k * ns : nullptr, grad_edge ? G * k * ns * 4 : 0);
  auto slot_of = [&](int c) { return (unsigned)(de_ldi(ags, up, c, n) & 0xff); };
  float av[G];
#pragma unroll
  for (int c = 0; c < G; ++c) av[c] = de_ldf(as, up, c, n);
  unsigned slot[C / 4];
#pragma unroll
  for (int c = 0; c < C / 4; ++c)
    slot[c] = slot_of(4 * c) | (slot_of(4 * c + 1) << 8) | (slot_of(4 * c + 2) << 16) | (slot_of(4 * c + 3) << 24);
  float ga[G], gc[LAST > 0 ? LAST * G : 1];
#pragma unroll
  for (int c = 0; c < G; ++c) ga[c] = 0.f;
#pragma unroll
  for (int c = 0; c < LAST * G; ++c) gc[c] = 0.f;
  float wacc[L > 0 ? T * T * (L * (L + 1) / 2) : 1];           // layer i at T*T*(i-1)*i/2, T x (i*T) row-major
#pragma unroll
  for (int c = 0; c < T * T * (L * (L + 1) / 2); ++c) wacc[c] = 0.f;
  const int r = t >> 3, q = t & 7;

  for (int j = 0; j < k; ++j) {
    const int src = min(max(de_ldi(is, up, j, n), 0), n - 1);
    const int nj = n + de_opaque_zero(__int_as_float(src));      // the rows' byte offsets: computed per slot, not kept
    float in[(LAST + 1) * G];
    const float *wj = w;
    de_edge_stack<G, LAST>(nbc + (size_t)src * G, av, cs, nj, up, wj, in);
    // grad_out routed to this slot (0 elsewhere)
    auto routed = [&](int c) {
      const bool here = live && ((slot[c >> 2] >> (8 * (c & 3))) & 0xffu) == (unsigned)j;
      const float g = de_ldf(gos, up, c, nj);
      return here ? g : 0.f;
    };
    float gin[(L > 0 ? L : 1) * G];                 // gradient at [edge; y_1 .. y_{L-1}] (post-activation)
#pragma unroll
    for (int c = 0; c < (L > 0 ? L : 1) * G; ++c) gin[c] = routed(c);
    if constexpr (L > 0) {
#pragma unroll
      for (int c = 0; c < L * G; ++c) s_in[t * kIn + c] = live ? in[c] : 0.f;
#pragma unroll
      for (int i = L; i >= 1; --i) {
        float gy[G];
#pragma unroll
        for (int c = 0; c < G; ++c) {
          if (i == L) {
            gy[c] = routed(L * G + c);
          } else {
            gy[c] = in[i * G + c] > 0.f ? gin[i * G + c] : 0.f;
            gc[(i - 1) * G + c] += gy[c];
          }
        }
        if (i == 2) de_layer<G, 2 * G, false>(wj + de_w_off(G, 2), gy, gin);      // gin[0 .. i*G) += W_i^T gy
        else de_layer<G, G, false>(wj + de_w_off(G, 1), gy, gin);
#pragma unroll
        for (int c = 0; c < G; ++c) s_gy[t * kGy + c] = gy[c];
        __syncthreads();
        // grad W_i block of this lane: rows r*T.., columns q*i*T..; the wave's 64 edges in ascending lane order
        float *wa = wacc + T * T * ((i - 1) * i / 2);
#pragma unroll 2
        for (int e = 0; e < kDeThreads; ++e) {
          float gr[T], xc[L * T];
#pragma unroll
          for (int u = 0; u < T; ++u) gr[u] = s_gy[e * kGy + r * T + u];
#pragma unroll
          for (int v = 0; v < i * T; ++v) xc[v] = s_in[e * kIn + q * i * T + v];
#pragma unroll
          for (int u = 0; u < T; ++u)
#pragma unroll
            for (int v = 0; v < i * T; ++v) wa[u * i * T + v] = __builtin_fmaf(gr[u], xc[v], wa[u * i * T + v]);
        }
        __syncthreads();                            // s_gy is rewritten by the next layer, s_in by the next slot
      }
    }
    if (live) {
#pragma unroll
      for (int c = 0; c < G; ++c) {
        gin[c] = in[c] > 0.f ? gin[c] : 0.f;        // the gradient at the pre-ReLU edge sum
        ga[c] += gin[c];
      }
      if (grad_edge) {                              // (null: nb is frozen, nobody scatters it)
#pragma unroll
        for (int c = 0; c < G; ++c) de_stf(ges, up, c * k + j, nj, gin[c]);
      }
    }
  }
  if (live) {
    const DeRsrc gas = de_slab(grad_a + (size_t)cloud * G * ns, G * ns * 4);
#pragma unroll
    for (int c = 0; c < G; ++c) de_stf(gas, up, c, n, ga[c]);
    if constexpr (L > 0) {
      const DeRsrc gcs = de_slab(grad_ctr + (size_t)cloud * L * G * ns, L * G * ns * 4);
#pragma unroll
      for (int c = 0; c < LAST * G; ++c) de_stf(gcs, up, c, n, gc[c]);
#pragma unroll
      for (int c = 0; c < G; ++c) de_stf(gcs, up, LAST * G + c, n, de_ldf(gos, up, L * G + c, n));   // exactly one slot is arg
    }
  }
  if constexpr (L > 0) {
    float *ps = partial + ((size_t)cloud * gridDim.x + blockIdx.x) * de_w_floats(G, L);
#pragma unroll
    for (int i = 1; i <= L; ++i)
#pragma unroll
      for (int u = 0; u < T; ++u)
#pragma unroll
        for (int v = 0; v < i * T; ++v)
          ps[de_w_off(G, i) + (r * T + u) * i * G + q * i * T + v] = wacc[T * T * ((i - 1) * i / 2) + u * i * T + v];
  }
}

// grad_w[e] = the slots' partial sums: chain s sums slots s, s + 8, .. ascending, then chains 0..7 ascending
constexpr int kDeRedChains = 8, kDeRedElems = 32;

__global__ __launch_bounds__(kDeRedChains *kDeRedElems) void dense_edge_conv_wsum_kernel(
    long long slots, int wfloats, const float *__restrict__ partial, float *__restrict__ grad_w) {
  __shared__ float s_sum[kDeRedChains][kDeRedElems];
  const int le = threadIdx.x % kDeRedElems, chain = threadIdx.x / kDeRedElems;
  const int e = blockIdx.x * kDeRedElems + le;
  float acc = 0.f;
  if (e < wfloats)
    for (long long s = chain; s < slots; s += kDeRedChains) acc += partial[(size_t)s * wfloats + e];
  s_sum[chain][le] = acc;
  __syncthreads();
  if (chain == 0 && e < wfloats) {
    float total = s_sum[0][le];
#pragma unroll
    for (int s = 1; s < kDeRedChains; ++s) total += s_sum[s][le];
    grad_w[e] = total;
  }
}

}  // namespace mvp

using namespace mvp;

#define MVP_DE_DISPATCH_L(G, LAUNCH)                                   \
  switch (layers) {                                                     \
    case 0: LAUNCH(G, 0); break;                                        \
    case 1: LAUNCH(G, 1); break;                                        \
    default: LAUNCH(G, 2); break;                                       \
  }
#define MVP_DE_DISPATCH(LAUNCH)                                         \
  switch (g) {                                                          \
    case 8: MVP_DE_DISPATCH_L(8, LAUNCH) break;                         \
    case 16: MVP_DE_DISPATCH_L(16, LAUNCH) break;                       \
    case 24: MVP_DE_DISPATCH_L(24, LAUNCH) break;                       \
    default: MVP_DE_DISPATCH_L(32, LAUNCH) break;                       \
  }

static long long de_slots(int b, int n) { return (long long)b * ((n + kDeThreads - 1) / kDeThreads); }

extern "C" long long mvp_dense_edge_conv_scratch_bytes(int b, int g, int layers, int k, int n) {
  if (!de_shape_ok(b, g, layers, k, n)) return 0;
  const long long bytes = 4ll * de_w_floats(g, layers) * de_slots(b, n);
  return bytes > 4 ? bytes : 4;            // layers == 0 or an empty batch need none; 0 stays "not covered"
}

extern "C" int mvp_dense_edge_conv(int b, int g, int layers, int k, int n, const float *a, const float *nb,
                                   const int *idx, const float *ctr, const float *w, float *out, int *arg,
                                   void *stream) {
  if (!de_shape_ok(b, g, layers, k, n)) return MVP_EBADSHAPE;
  if (b == 0 || n == 0) return MVP_OK;
  if (!a || !nb || !idx || !out || !arg || (layers > 0 && (!ctr || !w)) || misaligned(nb)) return MVP_EBADARG;
  const dim3 grid((n + kDeThreads - 1) / kDeThreads, b);
  hipStream_t st = as_stream(stream);
#define MVP_DE_FWD(G, L) \
  hipLaunchKernelGGL((dense_edge_conv_kernel<G, L>), grid, dim3(kDeThreads), 0, st, k, n, a, nb, idx, ctr, w, out, arg)
  MVP_DE_DISPATCH(MVP_DE_FWD)
#undef MVP_DE_FWD
  return check_launch("mvp_dense_edge_conv");
}

extern "C" int mvp_dense_edge_conv_grad(int b, int g, int layers, int k, int n, const float *a, const float *nb,
                                        const int *idx, const float *ctr, const float *w, const int *arg,
                                        const float *grad_out, float *grad_a, float *grad_edge, float *grad_ctr,
                                        float *grad_w, void *scratch, long long scratch_bytes, void *stream) {
  if (!de_shape_ok(b, g, layers, k, n)) return MVP_EBADSHAPE;
  if (b == 0 || n == 0) return MVP_OK;
  if (!a || !nb || !idx || !arg || !grad_out || !grad_a || misaligned(nb)) return MVP_EBADARG;
  if (layers > 0 && (!ctr || !w || !grad_ctr || !grad_w || !scratch ||
                     scratch_bytes < mvp_dense_edge_conv_scratch_bytes(b, g, layers, k, n)))
    return MVP_EBADARG;
  const dim3 grid((n + kDeThreads - 1) / kDeThreads, b);
  hipStream_t st = as_stream(stream);
  float *partial = static_cast<float *>(scratch);
#define MVP_DE_BWD(G, L)                                                                                              \
  hipLaunchKernelGGL((dense_edge_conv_grad_kernel<G, L>), grid, dim3(kDeThreads), 0, st, k, n, a, nb, idx, ctr, w, arg, \
                     grad_out, grad_a, grad_edge, grad_ctr, partial)
  MVP_DE_DISPATCH(MVP_DE_BWD)
#undef MVP_DE_BWD
  if (layers > 0) {
    const int wfloats = de_w_floats(g, layers);
    hipLaunchKernelGGL(dense_edge_conv_wsum_kernel, dim3((wfloats + kDeRedElems - 1) / kDeRedElems),
                       dim3(kDeRedChains * kDeRedElems), 0, st, de_slots(b, n), wfloats, partial, grad_w);
  }
  return check_launch("mvp_dense_edge_conv_grad");
}
