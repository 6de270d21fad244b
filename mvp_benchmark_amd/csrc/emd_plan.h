// The launch sequence of one mvp_emd_forward call, planned on the host: which kernels run, in which order, with which
// grid and scalar arguments.  Pure C++ -- no HIP call, no kernel, nothing read from the environment: emd.hip's executor
// asks emd_plan_next() for a step, launches it and reports whether the launch was accepted; tests/emd_plan_check.cpp
// walks the same function on the CPU.
//
// The knobs (process-wide: mvp_emd_configure; per call: MvpEmdPlan; libmvpops_hooks.so: MVP_EMD_* at first use).
// split: 0 one kernel runs every round; 1: the rounds after the last four-bidders-per-wave round run in the lean kernel
// (emd_lean.hip) on the first kernel's cluster width; 2: + cluster widths dealt out by load from round plan_round on
// (emd_lean_tiers_kernel; 33..64 clouds of >= 4096 points on width 4, launches of plan_every rounds); 3: + clouds of
// <= kResMaxN points finish LDS-resident on one workgroup once at most res_cap persons are unassigned, in a launch of
// their own (emd_resident.hip); 4: ... inside the lean launch, on member 0 of the cloud's cluster; 5 (default): +
// gathered-bid rounds.  The results do not depend on any of them (bit-identical; tests/test_gpu_ops.py).
//
// Three launches check the device's residency (cooperative launch) and may be REFUSED at run time; each has one answer:
//   the first kernel on W > 1     the first kernel on W = 1, plain launch, fast_ok 0; every later step sees w = 1
//   the fused resident lean       the same lean launch with RESN = 0; the resident launch follows either way
//   a tiered launch               the lean kernel on width 4 to the last round, on granule set 2; then done
// Any other launch that fails ends the plan (the executor returns the error).
#pragma once

namespace mvp {

// (device code reads these too: emd_common.h includes this header)
constexpr int kMaxCluster = 8;       // workgroups per cloud (W)
constexpr int kLeanMinRounds = 64;   // rounds that must be left for a hand-over to the lean kernel
constexpr int kResMaxN = 4096;       // points of a cloud the resident kernel takes
constexpr int kResList = 64;         // unassigned persons it takes over at most

// The bits of the kernels' `fast_ok` argument (the first kernel reads bit 0 only).
constexpr int kFastSameXcd = 1;       // members that find themselves on one XCD share its L2: plain stores
constexpr int kFastGathered = 2;      // gathered-bid rounds (split >= 5)
constexpr int kFastPollDistrust = 4;  // MVP_TEST_HOOKS builds: gathered-bid rounds of odd count re-read their bid records

struct EmdKnobs {
  int cluster, same_xcd, split;
  int plan_round, plan_every;     // split >= 2: round of the first tiered launch; rounds per tiered launch
  unsigned long long plan_widths; // widths of an XCD's 8 cloud slots, heaviest first, 4 bits each (0: from the loads)
  int res_cap;                    // split >= 3: unassigned persons at which a cloud of <= kResMaxN points moves into LDS
  int poll_distrust;              // MVP_TEST_HOOKS only: kFastPollDistrust
};
// The compiled-in defaults: of the process-wide knobs and of every mvp_emd_forward_plan call.
inline EmdKnobs emd_default_knobs() { return EmdKnobs{kMaxCluster, 1, 5, 300, 4096, 0ull, 16, 0}; }   // (MVP_EMD_PLAN_WIDTHS=8,5,4,4,3,3,3,2 fixes the widths)

enum EmdKernel { kEmdFirst, kEmdLean, kEmdTiers, kEmdResident };

// One launch.  grid, coop and the scalars are what goes to the device; W and resn select the instantiation.
struct EmdStep {
  EmdKernel kernel;
  int W, resn, grid;      // cluster width (tiers: the width its grid is sized for, 4; resident: 1); lean: 0 or the fused resident size, resident: its size (2048 / 4096)
  bool coop, refusable;   // cooperative launch (W > 1: cluster members wait for each other); a refusal has an answer (above)
  int lean, fast_ok, it_stop, which, u_stop;   // (those the kernel has)
  unsigned long long pattern;                  // tiers
};

struct EmdPlan {
  EmdKnobs k;
  int b, n, iters, cus;                // cus = 0 (the device query failed): width 1
  int w = 0, at = 0, r = 0;            // cluster width of the steps to come; emd_plan_next's position; tiers: rounds done
  unsigned long long pattern = 0ull;   // tiers: the widths (emd_plan_pattern)
  bool alt = false;                    // the step returned last was refusable
};

inline int emd_bpad(int b, int W) { return W == 1 ? b : (b + 7) / 8 * 8; }

// The tiered launches' widths: 0 = from the loads (the kernel), else plan_widths, heaviest first -- read only with 8 cloud
// slots per XCD.  false: not a pattern the kernel is instantiated for (each width one of 2, 3, 4, 5, 6, 8; sum = the XCD's
// 4 * bpad / 8 = 32 workgroups).
inline bool emd_plan_pattern(const EmdKnobs &k, int b, unsigned long long &pattern) {
  pattern = emd_bpad(b, 4) / 8 == 8 ? k.plan_widths : 0ull;
  int sum = 0;
  for (int s = 0; s < 8; ++s) {
    const int ws = (int)((pattern >> (4 * s)) & 15ull);
    sum += ws == 2 || ws == 3 || ws == 4 || ws == 5 || ws == 6 || ws == 8 ? ws : 64;
  }
  return pattern == 0ull || sum == 32;
}

// The next launch of the call, or false: done (or the last launch failed and had no answer).  `accepted`: whether the
// step returned before was launched (ignored on the first call).
inline bool emd_plan_next(EmdPlan &p, bool accepted, EmdStep &out) {
  enum { kStart, kFirst, kLeanResident, kTiers, kLast };
  const EmdKnobs &k = p.k;
  // the first kernel hands a cloud over when at least `lean` rounds are left (0: never)
  const int lean = k.split && p.iters > kLeanMinRounds ? kLeanMinRounds : 0;
  const int fast = (k.same_xcd ? kFastSameXcd : 0) | (k.split >= 5 ? kFastGathered : 0) | (k.poll_distrust ? kFastPollDistrust : 0);
  const int resn = p.n <= 2048 ? 2048 : 4096, cap = k.res_cap > kResList ? kResList : k.res_cap;
  const bool refused = p.at != kStart && !accepted;
  auto step = [&](int at, EmdKernel kernel, int W, int rn, bool alt, int it_stop, int which, int u_stop) {
    p.at = at;
    p.alt = alt && W > 1;   // (a plain launch is not refused)
    out = EmdStep{kernel, W, rn, W * emd_bpad(p.b, W), W > 1, p.alt, kernel == kEmdFirst ? lean : 0,
                  W == 1 ? 0 : kernel == kEmdFirst ? fast & kFastSameXcd : fast, it_stop, which, u_stop, kernel == kEmdTiers ? p.pattern : 0ull};
    return true;
  };
  if (refused && !p.alt) return false;
  switch (p.at) {
    case kStart:
      // workgroups per cloud: as many (1, 2, 4, 8; at most k.cluster) as keep b*W workgroups co-resident, one per CU
      for (p.w = 1; p.w * 2 <= k.cluster && p.w * 2 <= kMaxCluster && (long long)p.b * p.w * 2 <= p.cus;) p.w *= 2;
      return step(kFirst, kEmdFirst, p.w, 0, true, 0, 0, 0);
    case kFirst:
      if (refused) return step(kFirst, kEmdFirst, p.w = 1, 0, false, 0, 0, 0);   // (the cluster does not fit this device)
      if (!lean) return false;
      // (the resident branch is tested first: clouds of <= kResMaxN points are not dealt out again)
      if (k.split >= 3 && k.res_cap != 0 && p.n <= kResMaxN)
        return step(kLeanResident, kEmdLean, p.w, k.split >= 4 ? resn : 0, k.split >= 4, p.iters, 1, cap);
      // (below 4096 points a cloud has a few dozen bidders left at round 300: nothing to deal out -- measured: 2048 points +0.7 ms)
      if (p.w == 4 && p.n >= 4096 && p.b >= 33 && p.b <= 64 && k.split >= 2 && emd_plan_pattern(k, p.b, p.pattern) &&
          p.iters >= k.plan_round + 256)
        return step(kTiers, kEmdLean, 4, 0, false, p.r = k.plan_round, 1, 0);
      return step(kLast, kEmdLean, p.w, 0, false, p.iters, 1, 0);
    case kLeanResident:
      if (refused) return step(kLeanResident, kEmdLean, p.w, 0, false, p.iters, 1, cap);   // (only the fused launch is refusable)
      // (after a fused launch only clouds nobody finished -- none -- are left for it; it exits at once)
      return step(kLast, kEmdResident, 1, resn, false, 0, 0, 0);
    case kTiers:
      if (refused) return step(kLast, kEmdLean, 4, 0, false, p.iters, 2, 0);
      if (p.r == p.iters) return false;
      p.r = p.r + k.plan_every + 256 > p.iters ? p.iters : p.r + k.plan_every;   // (no short last launch)
      return step(kTiers, kEmdTiers, 4, 0, true, p.r, 2, 0);
  }
  return false;   // kLast
}

}  // namespace mvp
