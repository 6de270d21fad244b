// Measurement probes of the EMD auction kernels (emd.hip, emd_lean.hip and its fragments, emd_resident.h).  Everything the
// instrumented builds need lives here -- LDS arrays, per-thread counters, the reports -- and every probe in a kernel is ONE
// statement macro that expands to nothing in the release build:
//   -DMVP_EMD_PROFILE    (make prof)          EMD_PROF(...)   cycle counters and histograms, printed per cloud at the end
//                                                             (tools/bench_emd_one.py ... libmvpops_prof.so)
//   -DMVP_EMD_CLOUDTIME  (make variant ...)   EMD_CTIME(...)  per-cloud wall times in the last 64 words of the cloud's sc.chg
//                                                             (tools/emd_cloud_times.py)
//   -DMVP_EMD_GMTIME     (make variant ...)   GMT(i)          phase clock of the gathered-bid rounds in the 17 words at
//                                                             sc.chg[kMaxCluster * kChgCap - 128] (tools/emd_gm_times.py)
// A probe's argument is not evaluated in the release build (a cycle-counter read is a side effect the compiler keeps).
#pragma once
#include "emd_common.h"

#ifdef MVP_EMD_PROFILE
#define EMD_PROF(...) __VA_ARGS__
#else
#define EMD_PROF(...)
#endif
#ifdef MVP_EMD_CLOUDTIME
#define EMD_CTIME(...) __VA_ARGS__
#else
#define EMD_CTIME(...)
#endif
// Phase clock of the gathered-bid rounds as wave 0 of member 0 sees them (cycles, summed over the rounds): GMT(i) adds the
// time since the previous stamp to phase i.
#ifdef MVP_EMD_GMTIME
#define EMD_GMTIME(...) __VA_ARGS__
#define GMT(i) { const long long now_ = __builtin_readcyclecounter(); gmt[i] += now_ - gm_prev; gm_prev = now_; }
#else
#define EMD_GMTIME(...)
#define GMT(i)
#endif

namespace mvp {

// word of a cloud's CLOUDTIME area (tools/emd_cloud_times.py): cluster width | unassigned persons | ticks of the 100 MHz clock
__device__ __forceinline__ u64 emd_ctime_word(int w, int utot, long long ticks) {
  return ((u64)w << 48) | ((u64)utot << 32) | (u64)(unsigned)ticks;
}

#ifdef MVP_EMD_PROFILE
// LDS of the profile build (one object per workgroup).
struct EmdProbeLds {
  int s_wbusy[kEmdWaves];             // cycles of every wave's Bid phase this round
  unsigned long long s_hist2[4];      // sums per bid: seed cycles (high bits: price-bound refreshes), visit cycles, visit steps (high: contested), folds (high: flagged)
  float s_loose[2][3];                // [slow][sum of (seed threshold - final threshold), sum of seed threshold, -]
  unsigned long long s_slow[2][8];    // [d >= 10k cycles][count, nsub, cells, visit steps, extra member iterations, folds, seed cycles, visit cycles]
  unsigned long long s_hist[16];      // bids: [0..7] duration buckets, [8] sum nsub, [9] sum cells visited, [10] count, [11] linear scans, [12] sum cycles; [13..15] busiest wave, mean wave, rounds
  __device__ __forceinline__ void clear() {
    if (threadIdx.x < 4) s_hist2[threadIdx.x] = 0;
    if (threadIdx.x < 6) s_loose[threadIdx.x / 3][threadIdx.x % 3] = 0.f;
    if (threadIdx.x < 16) s_slow[threadIdx.x >> 3][threadIdx.x & 7] = 0;
    if (threadIdx.x < 16) s_hist[threadIdx.x] = 0;
  }
};

// Per-thread counters of a kernel's round loop.
struct EmdProbe {
  long long prof_gap = 0, prof_prev4 = 0;
  long long prof_pg1 = 0, prof_drain = 0, prof_gather = 0, cyc_bid = 0, cyc_sync1 = 0, cyc_assign = 0, cyc_sync2 = 0, n_alarm = 0,
            n_rebal = 0, prof_u = 0, prof_a1 = 0, prof_an = 0, prof_a2 = 0, prof_a3 = 0, prof_a4 = 0;
  long long t_loop0 = __builtin_readcyclecounter();

  // "head cloud 0" progress line at the given rounds
  __device__ __forceinline__ void head(bool first_kernel, int cloud, int wg, int it, int iters, int Utot) const {
    const bool early = first_kernel && (it == 1 || it == 2 || it == 3 || it == 5 || it == 10);
    if (cloud == 0 && wg == 0 && threadIdx.x == 0 &&
        (early || it == 25 || it == 50 || it == 100 || it == 150 || it == 250 || it == 500 || it == 750 || it == 1000 || it == 1500 ||
         it == 2000 || it == 2500 || it == iters - 1))
      printf("head cloud 0: round %d starts at %lld cycles, unassigned %d\n", it, __builtin_readcyclecounter() - t_loop0, Utot);
  }
  // thread 0, end of a one-bidder-per-wave round: the busiest and the mean wave of its Bid phase
  __device__ __forceinline__ void round_end(EmdProbeLds &pl, int U) {
    int mx = 0, sm = 0;
    for (int w = 0; w < kEmdWaves; ++w) { mx = max(mx, pl.s_wbusy[w]); sm += pl.s_wbusy[w]; }
    pl.s_hist[13] += mx; pl.s_hist[14] += sm / kEmdWaves; pl.s_hist[15] += 1; prof_u += U;
  }
};

// Counters of one bid's search (emd_search_wave.inc).
struct EmdBidProbe {
  long long tb0 = __builtin_readcyclecounter(), tb1 = tb0, t_visit = 0;
  float prof_tm_seed = 0.f;
  int n_visit = 0, prof_fold = 0, prof_more = 0, prof_cells = 0;

  // lane 0, after the search: the bid into the histograms.  tm_final >= 0: also the looseness of the seed threshold.
  __device__ __forceinline__ void done(EmdProbeLds &pl, int nsub, bool linear, float tm_final = -1.f) const {
    const long long d = __builtin_readcyclecounter() - tb0;
    int bkt = 0;
    while (bkt < 7 && d >= (2000ll << bkt)) ++bkt;
    atomicAdd(&pl.s_hist[bkt], 1ull);
    atomicAdd(&pl.s_hist[8], (unsigned long long)nsub);
    atomicAdd(&pl.s_hist[9], (unsigned long long)prof_cells);
    atomicAdd(&pl.s_hist[10], 1ull);
    if (linear) atomicAdd(&pl.s_hist[11], 1ull);
    atomicAdd(&pl.s_hist[12], (unsigned long long)d);
    atomicAdd(&pl.s_hist2[0], (unsigned long long)(tb1 - tb0));
    atomicAdd(&pl.s_hist2[1], (unsigned long long)t_visit);
    atomicAdd(&pl.s_hist2[2], (unsigned long long)n_visit);
    atomicAdd(&pl.s_hist2[3], (unsigned long long)prof_fold);
    if (tm_final >= 0.f) {
      atomicAdd(&pl.s_loose[d >= 10000 ? 1 : 0][0], prof_tm_seed - tm_final);
      atomicAdd(&pl.s_loose[d >= 10000 ? 1 : 0][1], prof_tm_seed);
    }
    unsigned long long *sl = pl.s_slow[d >= 10000 ? 1 : 0];
    atomicAdd(&sl[0], 1ull);
    atomicAdd(&sl[1], (unsigned long long)nsub);
    atomicAdd(&sl[2], (unsigned long long)prof_cells);
    atomicAdd(&sl[3], (unsigned long long)n_visit);
    atomicAdd(&sl[4], (unsigned long long)prof_more);
    atomicAdd(&sl[5], (unsigned long long)prof_fold);
    atomicAdd(&sl[6], (unsigned long long)(tb1 - tb0));
    atomicAdd(&sl[7], (unsigned long long)t_visit);
  }
};

// thread 0 of a workgroup, after the round loop: the report of emd_auction_kernel (lean = false) / emd_lean_body (lean = true)
__device__ __forceinline__ void emd_probe_report(bool lean, const EmdProbeLds &pl, const EmdProbe &pr, int cloud, int wg,
                                                 long long n_rounds, long long n_bids) {
  auto &s_hist = pl.s_hist; auto &s_hist2 = pl.s_hist2; auto &s_slow = pl.s_slow; auto &s_loose = pl.s_loose;
  if (cloud < 2)
    printf("cloud %d wg %d per wave-mode bid: seed %llu cycles, visits %llu cycles in %.2f steps folding %.1f candidates, rest (enumeration, finish) %llu\n", cloud, wg,
           s_hist2[0] / (s_hist[10] + 1), s_hist2[1] / (s_hist[10] + 1), (double)s_hist2[2] / (double)(s_hist[10] + 1), (double)s_hist2[3] / (double)(s_hist[10] + 1),
           (s_hist[12] - s_hist2[0] - s_hist2[1]) / (s_hist[10] + 1));
  if (cloud < 2)
    printf("cloud %d wg %d price-bound refreshes after round 100: %llu\n", cloud, wg, s_hist2[0] >> 40);
  if (cloud == 0 && wg == 0)
    for (int k = 0; k < 2; ++k) {
      const double c = (double)s_slow[k][0] + 1e-9;
      if (lean)
        printf("cloud 0 wg 0 searches %s 10k cycles: seed threshold %.3f cell widths, of which %.3f loose (seed - final)\n", k ? ">=" : "<",
               s_loose[k][1] / c, s_loose[k][0] / c);
      printf("cloud 0 wg 0 searches %s 10k cycles: %llu | mean sub-box %.0f cells, visited %.1f, visit steps %.2f, extra member iterations %.2f, folds %.1f, seed %.0f cycles, visits %.0f cycles\n",
             k ? ">=" : "<", s_slow[k][0], s_slow[k][1] / c, s_slow[k][2] / c, s_slow[k][3] / c, s_slow[k][4] / c, s_slow[k][5] / c, s_slow[k][6] / c, s_slow[k][7] / c);
    }
  if (cloud < 2 && lean)
    printf("cloud %d wg %d gathered rounds (thread 0, %lld): contest check %lld, settle body %lld, drain %lld, to barrier end %lld cycles per round; flagged %.2f contested %.3f per round\n", cloud, wg, pr.prof_an,
           pr.prof_a1 / (pr.prof_an + 1), pr.prof_a2 / (pr.prof_an + 1), pr.prof_a3 / (pr.prof_an + 1), pr.prof_a4 / (pr.prof_an + 1), (double)(s_hist2[3] >> 32) / (double)(pr.prof_an + 1), (double)(s_hist2[2] >> 32) / (double)(pr.prof_an + 1));
  if (cloud < 2 && !lean)
    printf("cloud %d wg %d Assign (thread 0, %lld samples): loads done at %lld cycles, eviction handled at %lld (sum over winning rounds / all), body done at %lld, phase %lld\n", cloud, wg, pr.prof_an, pr.prof_a1 / (pr.prof_an + 1), pr.prof_a2 / (pr.prof_an + 1), pr.prof_a3 / (pr.prof_an + 1), pr.prof_a4 / (pr.prof_an + 1));
  if (cloud < 2)
    printf("cloud %d wg %d tail rounds %llu: bidders/round %.1f, busiest wave %llu cycles/round, mean wave %llu\n", cloud, wg, s_hist[15],
           (double)pr.prof_u / (double)(s_hist[15] + 1), s_hist[13] / (s_hist[15] + 1), s_hist[14] / (s_hist[15] + 1));
  if (cloud < 2)
    printf("cloud %d wg %d wave-mode bids after round 100: %llu, mean cycles %llu, mean sub-box cells %llu, mean cells visited %llu, linear %llu | <2k %llu <4k %llu <8k %llu <16k %llu <32k %llu <64k %llu <128k %llu more %llu\n",
           cloud, wg, s_hist[10], s_hist[12] / (s_hist[10] + 1), s_hist[8] / (s_hist[10] + 1), s_hist[9] / (s_hist[10] + 1), s_hist[11],
           s_hist[0], s_hist[1], s_hist[2], s_hist[3], s_hist[4], s_hist[5], s_hist[6], s_hist[7]);
  if (cloud < 2 && lean)
    printf("cloud %d wg %d: rounds %lld bids %lld alarms %lld rebalances %lld | cycles bid %lld sync1 %lld assign %lld sync2 %lld gap %lld\n",
           cloud, wg, n_rounds, n_bids, pr.n_alarm, pr.n_rebal, pr.cyc_bid, pr.cyc_sync1, pr.cyc_assign, pr.cyc_sync2, pr.prof_gap);
  if (cloud < 2 && !lean)
    printf("cloud %d wg %d: rounds %lld bids %lld alarms %lld rebalances %lld | cycles bid %lld sync1 %lld assign %lld sync2 %lld \n",
           cloud, wg, n_rounds, n_bids, pr.n_alarm, pr.n_rebal, pr.cyc_bid, pr.cyc_sync1, pr.cyc_assign, pr.cyc_sync2);
  if (cloud < 2)
    printf("cloud %d wg %d: sync2 = store drain %lld + closing gather %lld + list bookkeeping %lld + bound fetch (rest)\n", cloud, wg, pr.prof_drain, pr.prof_gather, pr.prof_pg1);
}

// Counters of the resident rounds (emd_resident.h), per thread.
struct ResProbe {
  long long prof_folds = 0, prof_subs = 0, prof_bidcyc = 0, prof_nbid = 0, cyc_bid = 0, cyc_sync1 = 0, cyc_assign = 0, prof_slow = 0,
            prof_seed = 0;
  long long t_loop0 = __builtin_readcyclecounter();
  long long w_loop0 = wall_clock64();

  __device__ __forceinline__ void report(int cloud, int wave, int lane, long long n_rounds, long long n_bids) const {
    if (cloud < 2 && lane == 0 && (wave == 0 || wave == 3))
      printf("resident cloud %d wave %d: rounds %lld bids(all waves) %lld | this wave: %lld bids, %lld cycles each (home block %lld), sub-blocks %.1f folds %.1f per bid | cycles bid %lld wait %lld assign %lld total %lld | contested buckets %lld\n",
             cloud, wave, n_rounds, n_bids, prof_nbid, prof_bidcyc / (prof_nbid + 1), prof_seed / (prof_nbid + 1), (double)prof_subs / (double)(prof_nbid + 1),
             (double)prof_folds / (double)(prof_nbid + 1), cyc_bid, cyc_sync1, cyc_assign, __builtin_readcyclecounter() - t_loop0, prof_slow);
    if (cloud < 2 && lane == 0 && wave == 0)
      printf("resident cloud %d: %lld cycles in %lld ticks of the 100 MHz clock = %.0f MHz\n", cloud, __builtin_readcyclecounter() - t_loop0,
             wall_clock64() - w_loop0, 100.0 * (double)(__builtin_readcyclecounter() - t_loop0) / (double)(wall_clock64() - w_loop0));
  }
};
#define RES_PROF_ARGS , ResProbe &rp
#define RES_PROF_PASS , rp
#else
#define RES_PROF_ARGS
#define RES_PROF_PASS
#endif

}  // namespace mvp
