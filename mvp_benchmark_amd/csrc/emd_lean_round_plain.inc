// Part of emd_lean_body's round loop (csrc/emd_lean.hip), included INSIDE the loop body: PLAIN rounds after Bid -- the all-gather, GetMax when two increments met inside the 1e-6 band, Assign (emd_cuda.cu:181-215).
// every name used here is a local of emd_lean_body / of the `rounds` lambda (GM = gathered-bid rounds).
    alarm |= emd_band_alarm(pend_old, pend_inc);
    int *my_alarm = &s_alarm[it & 1];
    if (alarm) *my_alarm = 1;
    if (t == 0) s_cnt[cur ^ 1] = 0;
    // ---------------- all bids of the round are placed
    bool any_alarm;
    if (clustered) {
      // The bids themselves are complete (their atomics have returned); the
      // bidders' hint records are only read after the next draining gather.
      if (!emd_cluster_gather_n<WM, false>(slots, W, wg, ++epoch, my_alarm, my_alarm, s_gout, &s_abort, same_xcd)) {
        aborted = true;
        break;
      }
      any_alarm = false;
#pragma unroll
      for (int w = 0; w < WM; ++w) any_alarm |= w < W && s_gout[2 * w] != 0u;
    } else {
      __syncthreads();
      any_alarm = *my_alarm != 0;
    }

    // ---------------- GetMax (emd_cuda.cu:181-194): only when two different
    // increments within the 1e-6 band met on one object this round.  Every
    // bidder inside the band of the object's maximal increment raises the
    // key's bidder field; the increment field stays.
    if (__builtin_expect(any_alarm, 0)) {
      EMD_PROF(pr.n_alarm += 1;)
      for (int u = t; u < U; u += kEmdThreads) {
        const int j = s_bj[u], o = s_bo[u];
        const float bi = s_binc[u];
        const u64 key = sa.ld_key(o);
        if (emd_in_band(bi, emd_ord2f((unsigned)(key >> 32))))
          atomicMax(reinterpret_cast<u64 *>(&sc.ostate[o]), (key & 0xFFFFFFFF00000000ull) | (u64)((unsigned)j + 1u));
      }
      if (clustered) {
        if (!emd_cluster_gather_n<WM>(slots, W, wg, ++epoch, my_alarm, my_alarm, s_gout, &s_abort, same_xcd)) {
          aborted = true;
          break;
        }
      } else {
        __syncthreads();
      }
    }
    if (t == 0) {
      s_alarm[(it + 1) & 1] = 0;  // next round's flag; its writers are a barrier away
      s_next = kEmdWaves;         // list positions 0..15 belong to the waves, the rest are drawn
    }
    EMD_PROF(tp2 = __builtin_readcyclecounter();)

    // ---------------- Assign (emd_cuda.cu:196-215)
    u64 *my_chg = sc.chg + (size_t)wg * kChgCap;
    // Few bidders (the long tail): one or two per WAVE instead of all of them in
    // the lanes of wave 0 -- winners, losers and bound refreshes are divergent
    // paths with their own memory round trips, which a single wave would run
    // one after the other.  (Many bidders: consecutive lanes, conflict-free LDS.)
    const bool spread = U <= 4 * kEmdWaves * 4;
    // next round's list (position, or -1: no room -- cannot happen, the lists never outgrow the hand-over's)
    auto append = [&]() {
      const int pos = atomicAdd(&s_cnt[nxt], 1);
      if (__builtin_expect(pos >= kRecCap, 0)) {
        s_err = 1;
        return -1;
      }
      return pos;
    };
    for (int ub = 0; ub < U; ub += kEmdThreads) {
      const int u = ub + (spread ? lane * kEmdWaves + wave : t);
      if (u >= U) continue;
      const int j = s_bj[u], o = s_bo[u], b2k = s_b2k[u];
      const float bi = s_binc[u];
      EMD_PROF(const long long ta0 = __builtin_readcyclecounter();)
      const int4 os = sa.ld_ostate(o);
      const float4 oo = sa.ld_obj(o);  // independent of `os`: same round trip
      EMD_PROF(if (t == 0 && it >= 100) {
                 asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                 pr.prof_a1 += __builtin_readcyclecounter() - ta0;
                 pr.prof_an += 1;
               })
      if (last || (unsigned)os.x == (unsigned)j + 1u) {  // a loser may read after the winner reset the key to 0
        const int prev = os.z;
        if (!last && prev != -1) {
          // the evicted owner bids again next round, in this workgroup's list
          sa.st_i32(&ass[prev], -1);
          const int pos = append();
          if (__builtin_expect(pos >= 0, 1)) {
            {
              const float4 pa = sa.ld_person(prev, 0);
              const float4 pb = sa.ld_person(prev, 1);
              s_rq[nxt][pos] = pa;
              s_ri[nxt][pos] = make_int4(prev, __float_as_int(pb.y), __float_as_int(pb.z), 0);
            }
          }
        }
        EMD_PROF(if (t == 0 && it >= 100) { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); pr.prof_a2 += __builtin_readcyclecounter() - ta0; })
        sa.st_ostate(o, j);
        sa.st_i32(&ass[j], o);
        sa.st_f32(&sc.obj[o].w, oo.w + bi);
        // The leaf's price lower bound only changes when the object that just got dearer was (one
        // of) the cheapest of its leaf (the bounds are exact at this point, see the re-scan after
        // the closing barrier): report the leaf; every member of the cluster re-scans the reported
        // leaves once all of this round's prices are in memory.
        const int c = o >> lshift;
        if (oo.w <= l_lo[c].w) {
          const int q = atomicAdd(&s_nchg, 1);
          if (q < kLeanBid) s_own_chg[q] = c;
          if (clustered && q < kChgCap) {
            const u64 e = (u64)(unsigned)c << 32;
            if (same_xcd) __hip_atomic_store(my_chg + q, e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            else __hip_atomic_store(my_chg + q, e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
        }
      } else {
        // lost: stays in the list, record carried over through LDS
        const int pos = append();
        if (__builtin_expect(pos >= 0, 1)) {
          s_rq[nxt][pos] = s_rq[cur][u];
          s_ri[nxt][pos] = make_int4(j, o, b2k, 0);
        }
      }
      EMD_PROF(if (t == 0 && it >= 100) { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); pr.prof_a3 += __builtin_readcyclecounter() - ta0; })
    }
    EMD_PROF(tp3 = __builtin_readcyclecounter();
             if (t == 0 && it >= 100) pr.prof_a4 += tp3 - tp2;)
