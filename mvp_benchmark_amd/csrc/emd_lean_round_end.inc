// Part of emd_lean_body's round loop (csrc/emd_lean.hip), included INSIDE the loop body: end of a round -- next list sizes, hand-over / stop checks, collapse to member 0, rebalance, refreshed price bounds, entry into the gathered-bid rounds.
// every name used here is a local of emd_lean_body / of the `rounds` lambda (GM = gathered-bid rounds).
    // ---------------- end of round: next list sizes + refreshed price bounds
    if (GM || clustered) {   // (the gathered-bid rounds are a cluster's: the round that collapses it leaves them)
      EMD_PROF(long long tpd = tp3, tpg2 = tp3;)
      Utot = 0;
      bool overflow = false;
      int cntw[WM], chgw[WM];  // (the same for every lane: kept in scalar registers, the arithmetic on them is SALU work)
      if constexpr (!GM) {
        EMD_PROF(asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                 tpd = __builtin_readcyclecounter();)
        if (!emd_cluster_gather_n<WM>(slots, W, wg, ++epoch, &s_cnt[nxt], &s_nchg, s_gout, &s_abort, same_xcd)) {
          aborted = true;
          break;
        }
        EMD_PROF(tpg2 = __builtin_readcyclecounter();
                 pr.prof_drain += tpd - tp3;
                 pr.prof_gather += tpg2 - tpd;)
#pragma unroll
        for (int w = 0; w < WM; ++w) {
          cntw[w] = w < W ? __builtin_amdgcn_readfirstlane((int)s_gout[2 * w]) : 0;
          chgw[w] = w < W ? __builtin_amdgcn_readfirstlane((int)s_gout[2 * w + 1]) : 0;
          Utot += cntw[w];
          if (w != wg) overflow |= chgw[w] > kChgCap;
        }
      } else {
        // gathered-bid round: every member counted every member's next list itself
        {
          const int cv = s_gc[gnxt][lane & (kMaxCluster - 1)];   // (one LDS read; the rest is scalar work)
#pragma unroll
          for (int w = 0; w < WM; ++w) {
            cntw[w] = w < W ? __builtin_amdgcn_readlane(cv, w) : 0;
            chgw[w] = 0;
            Utot += cntw[w];
          }
          // the next round's bidders of this member and its first position in the cloud-wide order (this round's are
          // no longer needed); the length of the next list for the rounds that follow a collapse to member 0
          goff = 0;
#pragma unroll
          for (int w = 0; w + 1 < WM; ++w)
            if (w < wg) goff += cntw[w];
          gU = __builtin_amdgcn_readlane(cv, wg);
          if (t == 0) s_cnt[nxt] = gU;
        }
      }
      // (one test for all the events of a round's end: it_cold, u_cold in emd_lean.hip)
      if (__builtin_expect(it + 1 >= it_cold || Utot <= u_cold, 0)) {
        if constexpr (GM) {
          // the rounds end here (last round, or everybody assigned): what follows reads the other members' stores
          if (it + 1 >= iters || Utot == 0) {
            if (!emd_cluster_gather_n<WM>(slots, W, wg, ++epoch, &s_nchg, &s_nchg, s_gout, &s_abort, same_xcd)) {
              aborted = true;
              break;
            }
          }
        }
        if (__builtin_expect((it + 1 == it_stop && it + 1 < iters && Utot > 0) ||
                             (Utot <= u_stop && Utot > 0 && iters - (it + 1) >= kResMinRounds), 0)) {
          // ---- this launch's last round: the lists are left for the next launch below the loop
          stop_cnt = cntw[wg];
          stop_for_res = !(it + 1 == it_stop);
          break;
        }
        if (__builtin_expect(Utot > 0 && Utot <= kLeanSoloMax && it + 1 < iters, 0)) {
          // ---- hand everything to member 0 (lists of <= kSoloMax persons live
          // in LDS only: publish the person ids; their records are in memory)
          if (wg != 0 && t < cntw[wg]) sa.st_i32(my_ulist + t, s_ri[nxt][t].x);
          if (!emd_cluster_gather_n<WM>(slots, W, wg, ++epoch, &s_nchg, &s_nchg, s_gout, &s_abort, same_xcd)) {
            aborted = true;
            break;
          }
          if (wg != 0) {
            if (t == 0) atomicAdd(reinterpret_cast<unsigned long long *>(&stats[1]), (unsigned long long)n_bids);
            ret_early = true;
            return 0;
          }
          int idx = t;
#pragma unroll
          for (int w = 1; w < WM; ++w) {
            if (idx >= 0 && idx < cntw[w]) {
              const int jj = __hip_atomic_load(sc.ulist + (size_t)w * 2 * n + idx, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
              const float4 pa = sa.ld_person(jj, 0);
              const float4 pb = sa.ld_person(jj, 1);
              const int pos = atomicAdd(&s_cnt[nxt], 1);
              s_rq[nxt][pos] = pa;
              s_ri[nxt][pos] = make_int4(jj, __float_as_int(pb.y), __float_as_int(pb.z), 0);
            }
            idx -= cntw[w];
          }
          clustered = false;
          if constexpr (GM) sw = 3;
          if (t == 0) s_nchg = 0;
          __syncthreads();
        }
      }
      if (!GM && clustered) {
        // ---- rebalance: the round lasts as long as the fullest workgroup's
        // bid passes (16 bidders per pass, 64 in row mode).  When an even
        // split would need fewer passes than the fullest list does, lists
        // above their even share hand the surplus (their last entries) to the
        // lists below it.  Everybody derives the same plan from the gathered
        // counts; the ids travel through the donors' dead current lists.
        int maxc = 0;
#pragma unroll
        for (int w = 0; w < WM; ++w) maxc = max(maxc, cntw[w]);
        const int even = (Utot + W - 1) / W;
        const int cap = (even + 15) / 16 * 16;
        if (__builtin_expect(!gm && maxc > cap && it + 1 < iters, 0)) {
          const int base = Utot / W, rem = Utot % W;
          int exc[WM], dfc[WM], exoff = 0, dfoff = 0, my_exoff = 0, my_dfoff = 0;
#pragma unroll
          for (int w = 0; w < WM; ++w) {
            const int tgt = base + (w < rem ? 1 : 0);
            exc[w] = w < W ? max(0, cntw[w] - tgt) : 0;
            dfc[w] = w < W ? max(0, tgt - cntw[w]) : 0;
            if (w == wg) { my_exoff = exoff; my_dfoff = dfoff; }
            exoff += exc[w];
            dfoff += dfc[w];
          }
          (void)my_exoff;
          const int my_exc = exc[wg], my_dfc = dfc[wg], my_cnt = cntw[wg];
          int *dead = my_ulist + (size_t)cur * n;   // this round's list: no longer read
          for (int i = t; i < my_exc; i += kEmdThreads) {
            const int pos = my_cnt - my_exc + i;
            sa.st_i32(dead + i, s_ri[nxt][pos].x);
          }
          if (!emd_cluster_gather_n<WM>(slots, W, wg, ++epoch, &s_nchg, &s_nchg, s_gout, &s_abort, same_xcd)) {
            aborted = true;
            break;
          }
          for (int i = t; i < my_dfc; i += kEmdThreads) {
            int p = my_dfoff + i, jj = -1;   // p-th entry of the pool = donors' surpluses in order
#pragma unroll
            for (int w = 0; w < WM; ++w) {
              if (p >= 0 && p < exc[w])
                jj = __hip_atomic_load(sc.ulist + (size_t)w * 2 * n + (size_t)cur * n + p, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
              p -= exc[w];
            }
            const int pos = my_cnt + i;
            const float4 pa = sa.ld_person(jj, 0);
            const float4 pb = sa.ld_person(jj, 1);
            s_rq[nxt][pos] = pa;
            s_ri[nxt][pos] = make_int4(jj, __float_as_int(pb.y), __float_as_int(pb.z), 0);
          }
          if (t == 0) s_cnt[nxt] = my_cnt - my_exc + my_dfc;
          __syncthreads();
#pragma unroll
          for (int w = 0; w < WM; ++w) cntw[w] = w < W ? base + (w < rem ? 1 : 0) : 0;   // (every list is at its even share now)
          EMD_PROF(pr.n_rebal += 1;)
        }
      }
      EMD_PROF(const long long tpb = __builtin_readcyclecounter();
               pr.prof_pg1 += tpb - tpg2;)
      // the nodes' price bounds follow their leaves' (one lane per node, the last wave -- it seldom has a bidder; LDS
      // only, before this round's re-scans land: a bound that lags a round is still a bound)
      if (t >= kEmdThreads - kMaxNodes) emd_node_price(l_lo, n_lo, t - (kEmdThreads - kMaxNodes), nleaf);
      // re-scan of one leaf's prices (its first 16 members in ONE round trip: all of them up to 16384 points)
      auto rescan = [&](int leaf) {
        const int e0 = leaf << lshift, e1 = e0 + (1 << lshift);
        float pv[16], pm = __builtin_inff();
#pragma unroll
        for (int k = 0; k < 16; ++k) pv[k] = sa.ld_price(e0 + k);
#pragma unroll
        for (int k = 0; k < 16; ++k) pm = __builtin_fminf(pm, pv[k]);
        for (int s2 = e0 + 16; s2 < e1; ++s2) pm = __builtin_fminf(pm, sa.ld_price(s2));
        l_lo[leaf].w = pm;
      };
      if constexpr (GM) {
        // gathered-bid round: the leaf of every object won this round is re-scanned (this member stored all of
        // the round's prices itself and has drained them)
        const int pw = (int)(eg & 1u);
        const int nw = min(s_nwon[pw], kGCap);
        const int idx = kEmdThreads - 1 - t;
        if (idx < nw) rescan(s_won[pw][idx]);
      } else {
        // Exact price bounds: every leaf a winner of the cluster reported is re-scanned by every
        // member, from the prices in memory (all of this round's stores were drained before the
        // barrier opened).  The highest waves take the entries: they start bidding a little later,
        // the searches that run meanwhile may still see the old (lower, valid) bound.
        const int own_cnt = min(chgw[wg], kLeanBid);
        int idx = kEmdThreads - 1 - t, total = own_cnt;
        int cell = idx < own_cnt ? s_own_chg[idx] : -1;
        idx -= own_cnt;
        // (also in the round the cluster collapses to member 0: the others' last reports count)
#pragma unroll
        for (int w = 0; w < WM; ++w) {
          if (w == wg) continue;
          const int cnt = min(chgw[w], kChgCap);
          if (cell < 0 && idx >= 0 && idx < cnt)
            cell = (int)(__hip_atomic_load(sc.chg + (size_t)w * kChgCap + idx, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT) >> 32);
          idx -= cnt;
          total += cnt;
        }
        if (__builtin_expect(overflow || total > kEmdThreads || chgw[wg] > kLeanBid, 0)) {
          // (cannot happen with <= kLeanCap bidders per cloud) recompute every bound
          for (int c = t; c < nleaf; c += kEmdThreads) rescan(c);
        } else if (cell >= 0) {
          rescan(cell);
        }
      }
      if (t == 0) s_nchg = 0;
      // ---- at most kGCap persons left (and never more again): the rounds go on with gathered bids.  Every member's
      // view starts from the memory all of them agree on after the barrier above.
      if constexpr (WB != 1) {
        if (!GM && clustered && gm_ok && Utot <= kGCap && it + 1 < iters) {
          sw = 2;
          for (int s2 = t; s2 < n; s2 += kEmdThreads)
            s_owner[s2] = (unsigned short)__builtin_amdgcn_raw_buffer_load_b32(rs, ((unsigned)n + (unsigned)s2) * 16u + 8u, 0, 16);
#pragma unroll
          for (int w = 0; w < WM; ++w)
            if (t == w) {
              s_gc[0][w] = cntw[w];
              s_gc[1][w] = 0;
              s_gc[2][w] = 0;
            }
          gi = 0;
#pragma unroll
          for (int q = 0; q < 4; ++q)   // (the four counter areas: 1024 words each)
            reinterpret_cast<unsigned *>(&s_rq[0][0])[1024 + 2048 * q + t] = 0u;
          if (t == 0) {
            s_nwon[0] = 0;
            s_nwon[1] = 0;
            s_pub = 0;
          }
          __syncthreads();
        }
      }
    } else {
      __syncthreads();
      Utot = s_cnt[nxt];
      if (__builtin_expect((it + 1 == it_stop && it + 1 < iters && Utot > 0) ||
                           (Utot <= u_stop && Utot > 0 && iters - (it + 1) >= kResMinRounds), 0)) {   // (member 0 alone)
        stop_cnt = Utot;
        stop_for_res = !(it + 1 == it_stop);
        break;
      }
      {
        const int own_cnt = min(s_nchg, kLeanBid);
        __syncthreads();
        if (t == 0) s_nchg = 0;
        const int idx = kEmdThreads - 1 - t;
        if (t >= kEmdThreads - kMaxNodes) emd_node_price(l_lo, n_lo, t - (kEmdThreads - kMaxNodes), nleaf);
        if (idx < own_cnt) {
          const int leaf = s_own_chg[idx];
          float pm = __builtin_inff();
          for (int s2 = leaf << lshift; s2 < ((leaf + 1) << lshift); ++s2) pm = __builtin_fminf(pm, sa.ld_price(s2));
          l_lo[leaf].w = pm;
        }
      }
    }
    EMD_PROF(const long long tp4 = __builtin_readcyclecounter();
             pr.prof_prev4 = tp4;
             pr.cyc_bid += tp1 - tp0; pr.cyc_sync1 += tp2 - tp1; pr.cyc_assign += tp3 - tp2; pr.cyc_sync2 += tp4 - tp3;
             if (t == 0 && it >= 100) pr.round_end(pl, U);)
