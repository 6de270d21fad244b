// Part of emd_lean_body's round loop (csrc/emd_lean.hip), included INSIDE the loop body: GATHERED-BID rounds after Bid -- wait for the round's bid records, every member settles every bid (DESIGN.md 5.2b; emd_cuda.cu:181-215).
// every name used here is a local of emd_lean_body / of the `rounds` lambda (GM = gathered-bid rounds).
      // ---------------- gathered-bid round (DESIGN.md 5.2b): wait for the round's bids, then EVERY member settles ALL
      // of them on its own view of the cloud.  One cluster-wide wait per round: no bid atomic to wait for, no key to
      // read back, no closing barrier -- a member only ever reads what it wrote itself (prices: every member stores
      // every winner's new price, the same value) or what a heartbeat vouches for (hint records, written a round or
      // more before they are read).  emd_cuda.cu:181-215 (GetMax + Assign).
      if constexpr (WB != 1) {
        GMT(1)   // [1] own bids done
        u64 *ba = bid_area + (size_t)(eg & 1u) * kGStride;
        const unsigned T4 = eg % 15u + 1u, T6 = eg % 7u + 1u;
        u64 g0 = 0ull, g1 = 0ull;
        if (wave * kWave < Utot) {   // the waves of threads p < Utot: thread p takes bid p
          // (1) spin on the members' words of the round; the wave's bid records ride the same trip (their addresses are
          // known, the producer stores them before its word, each carries its own tags); (2) re-read the records whose
          // tags are not the round's -- rare: a record that arrived behind its member's word.
          // Every lane loads -- the lanes past the words / past the bids read the last one again: no branch between the
          // three loads, so they are in flight together and the word is tested as soon as it is there.
          const bool isb = t < Utot;
          const u64 *wp = ba + 2 * kGCap + (lane < W ? lane : W - 1), *rp = ba + 2 * (isb ? t : Utot - 1);
          for (unsigned spins = 0;; ++spins) {
            const u64 x = __hip_atomic_load(wp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            g0 = __hip_atomic_load(rp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            g1 = __hip_atomic_load(rp + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (__all(x == (u64)eg)) break;
            if (spins >= kSpinLimit) {
              if (lane == 0) s_abort = 1;
              EMD_PROF(if (lane < W) printf("cloud %d wg %d wave %d: member word %d stuck at %llu, want %u (it %d Utot %d U %d goff %d gi %d pub %d)\n", cloud, wg, wave, lane, x, eg, it, Utot, U, goff, gi, s_pub);)
              break;
            }
            __builtin_amdgcn_s_sleep(1);
          }
          GMT(2)   // [2] every member's word raised
          bool ok = !isb || ((unsigned)(g0 & 15ull) == T4 && (unsigned)(g1 & 7ull) == T6);
#ifdef MVP_TEST_HOOKS
          // MVP_EMD_POLL_DISTRUST=1 (fast_ok's kFastPollDistrust; libmvpops_hooks.so only): in rounds of odd eg the records that
          // came with the words count as untagged, so that the re-read below stays tested
          if ((fast_ok & 4) != 0 && (eg & 1u) != 0) ok = !isb;
#endif
          for (unsigned spins = 0;; ++spins) {
            if (isb && !ok) {
              g0 = __hip_atomic_load(ba + 2 * t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              g1 = __hip_atomic_load(ba + 2 * t + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              ok = (unsigned)(g0 & 15ull) == T4 && (unsigned)(g1 & 7ull) == T6;
            }
            if (__all(ok)) break;
            if (spins >= kSpinLimit) {
              if (lane == 0) s_abort = 1;
              EMD_PROF(if (!ok) printf("cloud %d wg %d: bid %d stuck: %llx %llx, want tags %u %u (it %d Utot %d U %d goff %d)\n", cloud, wg, t, g0, g1, T4, T6, it, Utot, U, goff);)
              break;
            }
            __builtin_amdgcn_s_sleep(1);
          }
        }
        GMT(3)   // [3] bids read
        // Everything of a bid's settlement that does not depend on the other bids is done here, in the shadow of the
        // wait for the round's last bid: who placed it, who owns the object now (the map only changes after the
        // barrier), where an evicted owner would go -- and, if to this member, the load of its record.
        int go = 0, gj = 0, gb2 = -1, gm_m = 0, prev = 0xFFFF;
        float ginc = 0.f, gnp = 0.f;
        float4 pa = make_float4(0.f, 0.f, 0.f, 0.f), pb = pa;
        if (t < Utot) {
          ginc = __uint_as_float((unsigned)(g0 >> 32));
          go = (int)(g0 >> 18) & 0x3FFF;
          gj = (int)(g0 >> 4) & 0x3FFF;
          gnp = __uint_as_float((unsigned)(g1 >> 32));
          gb2 = ((int)(g1 >> 17) & 0x7FFF) - 1;
          gm_m = (int)(g1 >> 3) & 7;
          s_go[t] = (unsigned short)go;
          s_gj[t] = (unsigned short)gj;
          s_ginc[t] = ginc;
          {
            unsigned char *bc = bid_count(go);
            atomicAdd(reinterpret_cast<unsigned *>(bc - (go & 3)), 1u << ((go & 3) * 8));
          }
          if (!last) {
            prev = s_owner[go];
            if (prev != 0xFFFF && t % W == wg) {
              pa = sa.ld_person(prev, 0);
              pb = sa.ld_person(prev, 1);
            }
          }
        }
        GMT(4)   // [4] decoded, owner looked up
        lds_barrier();
        GMT(5)   // [5] barrier after the poll
        if (s_abort) {
          aborted = true;
          break;
        }
        EMD_PROF(tp2 = __builtin_readcyclecounter();)
        int rec_pos = -1;
        // Bids for an object that got more than one bid (~0.3 per round at the headline): the wave settles one of
        // them at a time -- the maximal increment bid on the object, then the highest bidder inside its 1e-6 band
        // (emd_cuda.cu:181-194), over all of the round's bids, four per lane.
        int contested = 0;   // 1: another bid wins my object
        EMD_PROF(const long long tq0 = __builtin_readcyclecounter();)
        if (wave * kWave < Utot && !last) {
          bool flagged = false;
          if (t < Utot) {
            unsigned char *bc = bid_count(go);
            flagged = *bc != 1;
            *bc = 0;   // (a bid for the same object that reads after this sees 0: flagged as well)
          }
          unsigned long long fm = __ballot(flagged);
          EMD_PROF(if (lane == 0) atomicAdd(&pl.s_hist2[3], (unsigned long long)__builtin_popcountll(fm) << 32);)
          while (fm) {
            const int l = (int)__builtin_ctzll(fm);
            fm &= fm - 1ull;
            const int ol = __builtin_amdgcn_readlane(go, l), pl = (wave << 6) + l;
            const bool mine = flagged && go == ol;   // this wave's bids for the same object: settled together
            bool same = false;
            for (int q = lane; q < Utot; q += kWave) same |= q != pl && s_go[q] == ol;
            if (__builtin_expect(__any(same), 0)) {
              // a real contest: the maximal increment bid on the object, then the highest bidder inside its 1e-6 band
              // (emd_cuda.cu:181-194), over all of the round's bids, four per lane
              float mi = -__builtin_inff();
              for (int q = lane; q < Utot; q += kWave)
                if (s_go[q] == ol) mi = __builtin_fmaxf(mi, s_ginc[q]);
              mi = emd_wave_max(mi);
              float wjf = -1.f;   // (indices < 2^14: exact in float)
              for (int q = lane; q < Utot; q += kWave)
                if (s_go[q] == ol && emd_in_band(s_ginc[q], mi)) wjf = __builtin_fmaxf(wjf, (float)s_gj[q]);
              wjf = emd_wave_max(wjf);
              if (mine && (int)wjf != gj) contested = 1;   // (1: lost the contest)
              fm &= ~__ballot(mine);
            }
          }
        }
        EMD_PROF(const long long tq1 = __builtin_readcyclecounter();
                 if (contested) atomicAdd(&pl.s_hist2[2], 1ull << 32);)
        GMT(6)   // [6] contest check
        if (t < Utot) {
          const int m = gm_m;   // the member that placed bid t (it does the stores only one member needs to do)
          if (!contested) {
            if (!last) {
              s_owner[go] = (unsigned short)gj;
              sa.st_f32(&sc.obj[go].w, gnp);   // (every member: its own next searches read its own store)
              if (prev != 0xFFFF) {
                // the evicted owner bids again next round: in the list of member (position % W) -- the lists stay
                // even without any exchange
                const int d = t % W;
                const int pos = atomicAdd(&s_gc[gnxt][d], 1);
                if (d == wg) rec_pos = pos;
                if (m == wg) sa.st_i32(&ass[prev], -1);
              }
              s_won[eg & 1u][atomicAdd(&s_nwon[eg & 1u], 1)] = (unsigned short)(go >> lshift);
            }
            if (m == wg) {
              sa.st_ostate(go, gj);
              sa.st_i32(&ass[gj], go);
              if (last) sa.st_f32(&sc.obj[go].w, gnp);
            }
          } else {
            // lost: stays in its member's list, record carried over through LDS
            const int pos = atomicAdd(&s_gc[gnxt][m], 1);
            if (m == wg) {
              s_rq[nxt][pos] = s_rq[cur][t - goff];
              s_ri[nxt][pos] = make_int4(gj, go, gb2, 0);
            }
          }
        }
        GMT(7)   // [7] outcome applied (owner map, list positions, stores issued)
        // (what the next round starts from; nobody reads these before the barrier below.  By the last wave: it has
        // no bid to settle)
        if (t >= kEmdThreads - WM) s_gc[gzero][t - (kEmdThreads - WM)] = 0;
        if (t == kEmdThreads - 1) {
          s_nwon[(eg + 1u) & 1u] = 0;
          s_next = kEmdWaves;
          s_pub = 0;
        }
        // drain: this member's stores are performed before its next heartbeat says so (and before its own next
        // searches read the prices); the evicted persons' records have arrived
        EMD_PROF(const long long tq2 = __builtin_readcyclecounter();)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        EMD_PROF(const long long tq3 = __builtin_readcyclecounter();)
        GMT(8)   // [8] drained
        if (rec_pos >= 0) {
          s_rq[nxt][rec_pos] = pa;
          s_ri[nxt][rec_pos] = make_int4(prev, __float_as_int(pb.y), __float_as_int(pb.z), 0);
        }
        lds_barrier();
        GMT(9)   // [9] closing barrier
        EMD_PROF(tp3 = __builtin_readcyclecounter();
                 if (t == 0) { pr.prof_a1 += tq1 - tq0; pr.prof_a2 += tq2 - tq1; pr.prof_a3 += tq3 - tq2; pr.prof_a4 += tp3 - tq3; pr.prof_an += 1; })
      }
