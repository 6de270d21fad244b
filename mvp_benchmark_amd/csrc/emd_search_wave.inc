// One bidder on one wave: the pruned exact search for the best and second-best value (emd_cuda.cu:120-171 scans all n
// objects; see emd_index.h for the index and emd_common.h: kMargin for why every skip is lossless).  Included INSIDE the
// per-bidder loop of emd_auction_kernel's one-bidder-per-wave path (emd.hip) and of emd_lean_body (emd_lean_bid.inc).
// Names it expects from the including scope:
//   lane, qx, qy, qz (the bidder's point), hc (its home chunk), p1, p2 (slots of its previous best / second best or -1),
//   BidState st (b1 = b2 = -1e9, bk = b2k = -1 [, bp]), wl (this wave's list: 4 * kRowListCap unsigned shorts of LDS),
//   l_lo, l_hi, n_lo, n_hi (the index in LDS), n, nnode, lshift, kch (16-slot chunks per leaf), tpu, sc, sa.ld_obj(slot),
//   EMD_SEARCH_FOLD(mask, v, slot, price): emd_fold of the including kernel's flavour
// and, in the profile build, EmdBidProbe bp (emd_probe.h); nsub counts the leaves tested.
// Leaves `linear` (bool: the search scanned every object instead) defined for the statistics.
      const int sub = lane >> 4, sl = lane & 15;
      float nd2, npm;   // this lane's node: squared distance of the point to its box, its price bound (read in (1), tested in (2))
      // (1) Seed: the second-largest exact value among DISTINCT real objects is a lower bound B2 of the final second-best
      // value.  Four chunks of 16 slots, one per 16-lane row, in ONE memory round trip: the chunks of the previous best
      // and second-best objects (after a lost contest or an eviction the next best is usually one of their neighbours),
      // the bidder's home chunk and its sibling.  Duplicates are dropped (an object must not count twice).
      {
        // (the row's chunk and its validity from the bits of `sub`, all selects: a chain of `sub == r ? :` becomes a
        // switch, which is lowered to a tree of divergent branches -- 8 exec regions in front of the load)
        const int c1 = max(p1, -1) >> 4, c2 = max(p2, -1) >> 4;   // (-1 >> 4 == -1: no previous object)
        const int odd = sub & 1;
        const bool hi = sub >= 2;   // rows 2, 3: the home chunk hc and its sibling hc ^ 1
        const int cs = hi ? hc ^ odd : (odd ? c2 : c1);
        const bool sv = (hi | (cs >= 0)) & ((sub == 0) | (cs != c1)) & ((sub < 2) | (cs != c2));
        const float4 o = sa.ld_obj((sv ? cs : 0) * 16 + sl);   // (issued unconditionally: straight-line code up to the reduction)
        // (under the load's round trip: the part of the node test (2) that does not need the threshold)
        const float4 nlo = n_lo[lane], nhi = n_hi[lane];
        nd2 = emd_box_dist2(nlo, nhi, qx, qy, qz);
        npm = nlo.w;
        // (a row without a chunk of its own has loaded chunk 0: valued like the others -- no branch -- and dropped)
        const float val = emd_value(sqdist3(o.x - qx, o.y - qy, o.z - qz), o.w);
        const float v = sv ? val : -__builtin_inff();
        st.tm = (3.0f - emd_wave_second(v)) + kMargin;   // (the home chunk or the chunk that equals it is always there: >= 16 objects)
      }
      EMD_PROF(bp.tb1 = __builtin_readcyclecounter();
               bp.prof_tm_seed = st.tm;)
      // (2) the nodes: one lane each, one step
      unsigned long long nmask = __ballot(emd_box_reach(nd2, npm, st.tm));
      // When the whole cloud is within reach (high prices everywhere, e.g. a clustered prediction against a spread
      // target) the boxes only add overhead: every node passes AND so do all 64 leaves of the first step -> scan the
      // objects linearly, 4 x 64 per step, with the same lossless filter.  (Decided on the leaves, not on the nodes:
      // a node of 256 objects is within reach of many searches whose leaves then mostly fail.)
      bool all_near = __builtin_popcountll(nmask) >= nnode;
      bool linear = false;
      int nlist = 0;
      // (4) visit the listed leaves, 4 * kVisitLoads per step: each 16-lane row takes kVisitLoads leaves, so that many independent 16-byte loads per
      // lane are in flight at once and a typical bid (~6-10 surviving leaves) needs ONE dependent memory round trip here.
      auto visit = [&]() {
        EMD_PROF(const long long tv0 = __builtin_readcyclecounter();
                 bp.n_visit += (nlist + 4 * kVisitLoads - 1) / (4 * kVisitLoads);)
        for (int k0 = 0; k0 < nlist; k0 += 4 * kVisitLoads) {
          // (straight-line: the list entries are read unconditionally -- entries behind the list's end are
          // clamped and discarded -- so that they share ONE LDS round trip)
          int s[kVisitLoads];
          bool in[kVisitLoads];
#pragma unroll
          for (int r = 0; r < kVisitLoads; ++r) {
            const int cw = wl[min(k0 + r * 4 + sub, nlist - 1)];   // (behind the list's end: its last leaf again, loaded like the others and discarded)
            in[r] = k0 + r * 4 + sub < nlist;
            s[r] = (cw << lshift) + sl;
          }
          for (int c = 0; c < kch; ++c) {   // (one chunk per leaf up to 16384 points)
            float4 o[kVisitLoads];
#pragma unroll
            for (int r = 0; r < kVisitLoads; ++r)
              o[r] = sa.ld_obj(s[r] + 16 * c);
#pragma unroll
            for (int r = 0; r < kVisitLoads; ++r) {
              const float sd = sqdist3(o[r].x - qx, o[r].y - qy, o[r].z - qz);
              const float tq = st.tm - o[r].w;
              const bool ps = in[r] && tq >= 0.f && sd <= tq * tq;
              const unsigned long long m = __ballot(ps);
              EMD_PROF(bp.prof_fold += __builtin_popcountll(m);)
              if (m) EMD_SEARCH_FOLD(m, emd_value(sd, o[r].w), s[r] + 16 * c, o[r].w);
            }
          }
        }
        nlist = 0;
        EMD_PROF(bp.t_visit += __builtin_readcyclecounter() - tv0;)
      };
      // (3) the leaves of the passing nodes, four nodes per step (a 16-lane row each)
      while (nmask) {
        // the next four nodes as the bytes of one scalar (a node is a lane: < 64; 0xFF = none), a row takes its byte
        unsigned nd4 = 0u;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          nd4 |= (nmask ? (unsigned)__builtin_ctzll(nmask) : 0xFFu) << (8 * r);
          nmask &= nmask - 1ull;
        }
        const unsigned nb = (nd4 >> (8 * sub)) & 0xFFu;
        const int node = nb == 0xFFu ? -1 : (int)nb;
        const int leaf = max(node, 0) * kNodeFan + sl;
        const bool lpass = (node >= 0) & emd_box_pass<true>(l_lo[leaf], l_hi[leaf], qx, qy, qz, st.tm);
        const unsigned long long lm = __ballot(lpass);
        if (__builtin_expect(all_near && lm == ~0ull, 0)) {
          linear = true;
          break;
        }
        all_near = false;
        if (lpass) wl[nlist + __builtin_popcountll(lm & ((1ull << lane) - 1ull))] = (unsigned short)leaf;
        nlist += __builtin_popcountll(lm);
        EMD_PROF(nsub += 64;
                 bp.prof_cells += __builtin_popcountll(lm);)
        if (nlist > 4 * kRowListCap - kWave) visit();   // keep room for the next step's 64 leaves
      }
      if (__builtin_expect(linear, 0)) {
        for (int base = 0; base < n; base += 4 * kWave) {
          float4 o[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) o[r] = sa.ld_obj(base + r * kWave + lane);  // n % 1024 == 0
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float sd = sqdist3(o[r].x - qx, o[r].y - qy, o[r].z - qz);
            const float tq = st.tm - o[r].w;
            const bool ps = tq >= 0.f && sd <= tq * tq;
            const unsigned long long m = __ballot(ps);
            if (m) EMD_SEARCH_FOLD(m, emd_value(sd, o[r].w), base + r * kWave + lane, o[r].w);
          }
        }
      }
      visit();
