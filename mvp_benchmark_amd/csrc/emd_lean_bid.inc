// Part of emd_lean_body's round loop (csrc/emd_lean.hip), included INSIDE the loop body: the Bid phase -- one wave per bidder: the search (emd_search_wave.inc), then the bid itself (emd_cuda.cu:95-179).
// every name used here is a local of emd_lean_body / of the `rounds` lambda (GM = gathered-bid rounds).
    // ---------------- Bid (emd_cuda.cu:95-179): one wave per bidder
    // Every bidder's record is in LDS (a list never outgrows the hand-over's <= kLeanCap
    // persons).  Bids differ in length (4k to 16k cycles), so a wave that finishes draws the
    // next list position from a shared counter instead of owning every 16th one: the phase
    // lasts sum / 16 instead of the longest pair.  (The loop is bounded independently of the
    // drawn position.)
    int u = wave;
    for (int guard = 0; guard <= kRecCap && u < U; ++guard) {
      const float4 ra = s_rq[cur][u];
      const int4 rb = s_ri[cur][u];
      int drawn = 0;
      const int j = rb.x;
      const float qx = ra.x, qy = ra.y, qz = ra.z;
      const int p1 = rb.y, p2 = rb.z;
      EMD_PROF(EmdBidProbe bp;)
      const int hc = __float_as_int(ra.w);   // home chunk (emd_index.h)
      BidState st;
      st.b1 = -1e9f;
      st.b2 = -1e9f;
      st.bk = -1;
      st.b2k = -1;
      st.bp = 0.f;
      unsigned short *wl = w_list[wave];
      int nsub = 0;          // leaves tested (statistics)
#define EMD_SEARCH_FOLD(m_, v_, slot_, price_) emd_fold<GM>(st, m_, v_, slot_, n, tpu, sc.perm, price_)
#include "emd_search_wave.inc"
#undef EMD_SEARCH_FOLD
      (void)nsub;
      EMD_PROF(if (lane == 0 && it >= 100) bp.done(pl, nsub, linear, (3.0f - st.b2) + kMargin);)
      if (st.bk < 0) {  // cannot happen (>= 2 objects always survive); never index with -1
        if (lane == 0) s_err = 1;
        st.bk = 0;
        st.b2k = -1;
      }
      if (lane == 0) {
        const float inc = st.b1 - st.b2 + eps;
        sa.st_person_hi(j, st.bk, st.bk, st.b2k, inc);
        if constexpr (GM) {
          // The bid as a granule at this bidder's position of the cloud-wide order: two 8-byte words, each with a
          // tag of the round -- {increment | object 14 | bidder 14 | tag 4}, {the object's new price | second-best
          // slot + 1 (next round's hint) 15 | 11 bits unused (the grid's cell; the leaf is the object's slot >> 4) | the bidder's member 3 | tag 3} -- so that every member can settle it without
          // reading anything else.  (A position below the cloud's bidder count is rewritten every round of its
          // parity: the tags only have to tell a round from the one two before.)
          const float np = st.bp + inc;
          const u64 g0 = ((u64)__float_as_uint(inc) << 32) | ((u64)(unsigned)st.bk << 18) | ((u64)(unsigned)j << 4) |
                         (u64)(eg % 15u + 1u);
          const u64 g1 = ((u64)__float_as_uint(np) << 32) | ((u64)(unsigned)(st.b2k + 1) << 17) |
                         ((u64)(unsigned)wg << 3) | (u64)(eg % 7u + 1u);
          u64 *slot = bid_area + (size_t)(eg & 1u) * kGStride + 2 * (size_t)(goff + u);
          if (same_xcd) {
            __hip_atomic_store(slot, g0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_store(slot + 1, g1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          } else {
            __hip_atomic_store(slot, g0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(slot + 1, g1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
          // The member's word of the round ("all my bids are out; everything I stored in earlier rounds is performed"
          // -- the previous settle ended with a drain): raised with the member's last bid.  It is what the others
          // spin on (W words per poll instead of every bid: polling the bids themselves by every waiting wave of 256
          // CUs saturated the L2 and doubled the round); only a hint for the bids -- each carries its own tags.
          if (atomicAdd(&s_pub, 1) == U - 1) {
            u64 *hb = bid_area + (size_t)(eg & 1u) * kGStride + 2 * kGCap + wg;
            if (same_xcd) __hip_atomic_store(hb, (u64)eg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            else __hip_atomic_store(hb, (u64)eg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
        } else {
          s_bj[u] = j;
          s_bo[u] = st.bk;
          s_b2k[u] = st.b2k;
          s_binc[u] = inc;
          alarm |= emd_band_alarm(pend_old, pend_inc);
          pend_old = atomicMax(reinterpret_cast<u64 *>(&sc.ostate[st.bk]),
                               ((u64)emd_f2ord(inc) << 32) | (u64)((unsigned)j + 1u));
          pend_inc = inc;
        }
        drawn = atomicAdd(&s_next, 1);
      }
      u = __builtin_amdgcn_readlane(drawn, 0);
    }
