// Part of emd_lean_body (csrc/emd_lean.hip), included as the body of the `few` lambda: the rounds of a cloud that is
// down to at most kEmdWaves (16) unassigned persons, on member 0 alone, until the auction ends (emd_cuda.cu:95-215).
// every name used here is a local of emd_lean_body.
//
// The plain rounds of a collapsed cluster cost ~16k cycles with ~8 bidders (profile build, chair gt + noise at 16384
// points): the slowest search 7.8k, then three workgroup barriers and FOUR dependent memory round trips after it --
// the object's key and price, the evicted owner's record, the drain of the stores, the re-scan of the leaf's prices.
// A prediction close to its ground truth spends 75-90 % of its 3000 rounds here (oracle trace, NOTES_r6 section 17).
// This loop is the LDS-resident tail's round (emd_resident.h) around the index search of the clustered kernels:
//   * a list position -- a wave -- holds its bidder's record in registers for the life of the loop: a loser stays,
//     an evicted owner takes the place of the winner that evicted it, a winner of a free object leaves it empty;
//   * Bid: the wave's search (emd_search_wave.inc; objects in memory, boxes and price bounds in LDS); the bid goes to LDS,
//     counted in a 256-bucket table; the 16 prices of the best object's leaf are requested before the barrier;
//   * GetMax + Assign: the wave settles its own bid after ONE barrier: a count of one = nobody else bid (else the bids
//     in LDS are compared: maximal increment, then the highest bidder inside its 1e-6 band, emd_cuda.cu:181-194);
//     the owner map is in LDS (s_owner), the object's price is the one the search read (prices do not move during
//     Bid), the leaf's price bound = the minimum of the prices requested above with the new price put in (a second
//     winner in the same leaf reads the other's OLD price: a lower, still valid bound), its node's bound follows;
//     price, owner and assignment are stored (nobody reads them back in the round); the owner's record was requested
//     BEFORE the barrier (the owner map does not change during Bid) and becomes the wave's next bidder; the closing
//     barrier waits for the stores' acknowledgement -- the one memory round trip after the search.
// Same bids, same winners, same prices as the plain rounds (which remain: launches that stop before the last round,
// clouds above kGMaxN points, MVP_EMD_FEW=0).
  constexpr int P = kFewPos;   // list positions per wave: wave w holds positions w, w + 16, ...
  const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
  auto &f_cnt = sh.f_cnt;
  auto &f_act = sh.f_act;
  int fj[P], fp1[P], fp2[P], fhc[P];
  float fqx[P], fqy[P], fqz[P];
  {
    const int U0 = s_cnt[cur];
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int pos = wv + p * kEmdWaves;
      fj[p] = -1; fp1[p] = -1; fp2[p] = -1; fhc[p] = 0;
      fqx[p] = 0.f; fqy[p] = 0.f; fqz[p] = 0.f;
      if (pos < U0) {
        const float4 ra = s_rq[cur][pos];
        const int4 rb = s_ri[cur][pos];
        fj[p] = __builtin_amdgcn_readfirstlane(rb.x);
        fp1[p] = __builtin_amdgcn_readfirstlane(rb.y);
        fp2[p] = __builtin_amdgcn_readfirstlane(rb.z);
        fhc[p] = __builtin_amdgcn_readfirstlane(__float_as_int(ra.w));
        fqx[p] = ra.x;
        fqy[p] = ra.y;
        fqz[p] = ra.z;
      }
    }
    if (t < 2 * 256) (&f_cnt[0][0])[t] = 0;
    if (t == 0) {
      f_act[it % 3] = U0;
      f_act[(it + 1) % 3] = 0;
      f_act[(it + 2) % 3] = 0;
    }
    // the owner map: the gathered-bid rounds keep it (every member's view); after plain rounds it is read from the
    // objects' records (every store of the last round is performed: the round ended with a drain and a barrier)
    if (!owners_in_lds)
      for (int s2 = t; s2 < n; s2 += kEmdThreads) s_owner[s2] = (unsigned short)sa.ld_ostate(s2).z;
    __syncthreads();
  }
  unsigned short *wl = w_list[wv];
  const int sl16 = lane & 15;
  EMD_PROF(long long fw_bid = 0, fw_wait = 0, fw_settle = 0, fw_close = 0, fw_rounds = 0, fw_mybids = 0, fw_search = 0;)
  for (; it < iters; ++it) {
    EMD_PROF(const long long fw0 = __builtin_readcyclecounter();)
    const int U = __builtin_amdgcn_readfirstlane(f_act[it % 3]);
    if (U == 0) break;
    Utot = U;
    n_rounds += 1;
    n_bids += U;
    const bool last = it == iters - 1;
    const int tpu = -U;   // (resolved inside emd_precedes: only equal values ever need it)
    int *cnt = f_cnt[it & 1];
    int bko[P], b2ko[P], prevo[P];
    float inco[P], npo[P], pwo[P];
    float4 pa[P], pb[P];
    // ---------------- Bid (emd_cuda.cu:95-179): the wave's positions one after the other
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int pos = wv + p * kEmdWaves;
      bko[p] = 0; b2ko[p] = -1; inco[p] = 0.f; npo[p] = 0.f; pwo[p] = 0.f;
      prevo[p] = 0xFFFF;
      pa[p] = make_float4(0.f, 0.f, 0.f, 0.f);
      pb[p] = pa[p];
      if (fj[p] >= 0) {
        BidState st;
        st.b1 = -1e9f;
        st.b2 = -1e9f;
        st.bk = -1;
        st.b2k = -1;
        st.bp = 0.f;
        const float qx = fqx[p], qy = fqy[p], qz = fqz[p];
        const int hc = fhc[p], p1 = fp1[p], p2 = fp2[p];
        int nsub = 0;
        EMD_PROF(EmdBidProbe bp;)
#define EMD_SEARCH_FOLD(m_, v_, slot_, price_) emd_fold<true>(st, m_, v_, slot_, n, tpu, sc.perm, price_)
#include "emd_search_wave.inc"
#undef EMD_SEARCH_FOLD
        (void)nsub;
        (void)linear;
        EMD_PROF(fw_search += __builtin_readcyclecounter() - fw0;
                 fw_mybids += 1;)
        if (st.bk < 0) {  // cannot happen (>= 2 objects always survive); never index with -1
          if (lane == 0) s_err = 1;
          st.bk = 0;
          st.b2k = -1;
        }
        const float inc = st.b1 - st.b2 + eps;
        bko[p] = st.bk;
        b2ko[p] = st.b2k;
        inco[p] = inc;
        npo[p] = st.bp + inc;
        pwo[p] = sa.ld_price((st.bk & ~15) + sl16);   // the leaf's prices as they are during Bid (used if the bid wins)
        // ... and the record of the object's owner (the map does not change during Bid), requested NOW: if the bid wins --
        // nearly always -- the evicted owner's point and hints have arrived by the time the barrier opens
        if (!last) {
          prevo[p] = __builtin_amdgcn_readfirstlane((int)s_owner[st.bk]);
          if (prevo[p] != 0xFFFF) {
            pa[p] = sa.ld_person(prevo[p], 0);
            pb[p] = sa.ld_person(prevo[p], 1);
          }
        }
        if (lane == 0) {
          sa.st_person_hi(fj[p], st.bk, st.bk, st.b2k, inc);
          s_bj[pos] = fj[p];
          s_bo[pos] = st.bk;
          s_binc[pos] = inc;
          atomicAdd(&cnt[st.bk & 255], 1);
        }
      } else if (lane == 0) {
        s_bj[pos] = -1;
      }
    }
    EMD_PROF(const long long fw1 = __builtin_readcyclecounter();)
    lds_barrier();
    EMD_PROF(const long long fw2 = __builtin_readcyclecounter();)
    if (last) {
      // the forced last round (emd_cuda.cu:201-212): every bidder takes the object it bid on
#pragma unroll
      for (int p = 0; p < P; ++p)
        if (fj[p] >= 0 && lane == 0) {
          sa.st_ostate(bko[p], fj[p]);
          sa.st_i32(&ass[fj[p]], bko[p]);
          sa.st_f32(&sc.obj[bko[p]].w, npo[p]);
        }
      break;
    }
    // ---------------- GetMax + Assign (emd_cuda.cu:181-215): every wave settles the bids it placed
    bool wino[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
      wino[p] = false;
      if (fj[p] >= 0) {
        const int bk = bko[p];
        bool win = true;
        if (__builtin_expect(__builtin_amdgcn_readfirstlane(cnt[bk & 255]) != 1, 0)) {
          // another bid in my bucket: the maximal increment bid on my object, then the highest bidder inside its band
          const bool on = lane < P * kEmdWaves && s_bj[lane] >= 0 && s_bo[lane] == bk;
          const float mi = emd_wave_max(on ? s_binc[lane] : -__builtin_inff());
          const float wjf = emd_wave_max(on && emd_in_band(s_binc[lane], mi) ? (float)s_bj[lane] : -1.f);   // (indices < 2^14: exact)
          win = (int)wjf == fj[p];
        }
        wino[p] = win;
      }
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
      if (fj[p] >= 0) {
        const int bk = bko[p];
        if (wino[p]) {
          const int prev = prevo[p];
          const int leaf = bk >> 4;
          const float pm = row_min(sl16 == (bk & 15) ? npo[p] : pwo[p]);
          // the node's bound from its leaves' (this leaf's new one put in)
          const float lw = l_lo[(leaf & ~(kNodeFan - 1)) + sl16].w;
          const float nm = row_min(sl16 == (leaf & (kNodeFan - 1)) ? pm : (((leaf & ~(kNodeFan - 1)) + sl16) < nleaf ? lw : __builtin_inff()));
          if (lane == 0) {
            s_owner[bk] = (unsigned short)fj[p];
            l_lo[leaf].w = pm;
            n_lo[leaf / kNodeFan].w = nm;
            sa.st_f32(&sc.obj[bk].w, npo[p]);
            sa.st_ostate(bk, fj[p]);
            sa.st_i32(&ass[fj[p]], bk);
            if (prev != 0xFFFF) sa.st_i32(&ass[prev], -1);
          }
          if (prev != 0xFFFF) {   // the evicted owner bids next round, from this position
            fj[p] = prev;
            fqx[p] = pa[p].x;
            fqy[p] = pa[p].y;
            fqz[p] = pa[p].z;
            fhc[p] = __builtin_amdgcn_readfirstlane(__float_as_int(pa[p].w));
            fp1[p] = __builtin_amdgcn_readfirstlane(__float_as_int(pb[p].y));
            fp2[p] = __builtin_amdgcn_readfirstlane(__float_as_int(pb[p].z));
          } else {
            fj[p] = -1;
          }
        } else {   // lost: bids again, seeded by what it just found
          fp1[p] = bk;
          fp2[p] = b2ko[p];
        }
        if (fj[p] >= 0 && lane == 0) atomicAdd(&f_act[(it + 1) % 3], 1);
      }
    }
    if (wv == kEmdWaves - 1) {
      // the next round's counters (last read in the round before this one), the count of the round after next
      reinterpret_cast<int4 *>(f_cnt[(it + 1) & 1])[lane] = make_int4(0, 0, 0, 0);
      if (lane == 0) f_act[(it + 2) % 3] = 0;
    }
    EMD_PROF(const long long fw3 = __builtin_readcyclecounter();)
    __syncthreads();   // (also: the stores are performed -- the next searches read the prices -- and the record has arrived)
    EMD_PROF(const long long fw4 = __builtin_readcyclecounter();
             fw_bid += fw1 - fw0; fw_wait += fw2 - fw1; fw_settle += fw3 - fw2; fw_close += fw4 - fw3; fw_rounds += 1;)
  }
  EMD_PROF(if (cloud < 2 && lane == 0 && (wv == 0 || wv == 5) && fw_rounds > 0)
             printf("few-bidder rounds cloud %d wave %d: %lld rounds from round %d | per round: bid phase %lld, wait at barrier %lld, settle %lld, closing barrier (stores + record) %lld cycles | this wave: %lld bids, search %lld cycles each\n",
                    cloud, wv, fw_rounds, (int)(it - fw_rounds), fw_bid / fw_rounds, fw_wait / fw_rounds, fw_settle / fw_rounds, fw_close / fw_rounds, fw_mybids, fw_search / (fw_mybids + 1));)
