// Prints the launch sequence mvp_emd_forward plans (csrc/emd_plan.h) for a list of cases, one line per launch.
// Host only: no HIP call, no kernel.  tests/test_emd_plan_cpu.py compiles it, runs it and compares the output with
// traces written out by hand from the launch rules.
//   c++ -std=c++17 -I mvp_benchmark_amd/csrc tests/emd_plan_check.cpp -o emd_plan_check && ./emd_plan_check
#include <cstdio>
#include <initializer_list>

#include "emd_plan.h"

using namespace mvp;

// The widths of an XCD's 8 cloud slots, heaviest first, as MVP_EMD_PLAN_WIDTHS packs them: 4 bits each.
static unsigned long long widths(std::initializer_list<int> ws) {
  unsigned long long pat = 0ull;
  int s = 0;
  for (int w : ws) pat |= (unsigned long long)(w & 15) << (4 * s++);
  return pat;
}

// `refuse`: bit i set = the i-th launch of the call is refused.
static void run(const char *name, const EmdKnobs &k, int b, int n, int iters = 3000, int cus = 256, unsigned refuse = 0u) {
  std::printf("== %s\n", name);
  EmdPlan plan{k, b, n, iters, cus};
  EmdStep s;
  bool ok = true;
  for (int i = 0; emd_plan_next(plan, ok, s); ++i) {
    const char *launch = s.coop ? "coop" : "plain";
    switch (s.kernel) {
      case kEmdFirst:
        std::printf("first W%d %s grid %d lean %d fast_ok %d", s.W, launch, s.grid, s.lean, s.fast_ok);
        break;
      case kEmdLean:
        std::printf("lean W%d RESN %d %s grid %d fast_ok %d it_stop %d which %d u_stop %d", s.W, s.resn, launch, s.grid,
                    s.fast_ok, s.it_stop, s.which, s.u_stop);
        break;
      case kEmdTiers:
        std::printf("tiers W%d %s grid %d fast_ok %d it_stop %d which %d pattern 0x%llx", s.W, launch, s.grid, s.fast_ok,
                    s.it_stop, s.which, s.pattern);
        break;
      case kEmdResident:
        std::printf("resident RESN %d %s grid %d", s.resn, launch, s.grid);
        break;
    }
    ok = ((refuse >> i) & 1u) == 0u;
    std::printf("%s\n", ok ? "" : s.refusable ? " -> refused" : " -> refused, no answer");
  }
  if (!ok) std::printf("error\n");
}

int main() {
  const EmdKnobs d = emd_default_knobs();
  auto with = [&](int split, int cluster = -1, int res_cap = -1) {
    EmdKnobs k = d;
    k.split = split;
    if (cluster > 0) k.cluster = cluster;
    if (res_cap > 0) k.res_cap = res_cap;
    return k;
  };
  run("1 b64 n16384", d, 64, 16384);
  run("2 b64 n16384 tiers refused", d, 64, 16384, 3000, 256, 1u << 2);
  run("3 b64 n16384 first refused", d, 64, 16384, 3000, 256, 1u << 0);
  run("4 b2 n4096", d, 2, 4096);
  run("5 b2 n4096 fused refused", d, 2, 4096, 3000, 256, 1u << 1);
  run("5b b2 n4096 fused refused, then the plain lean launch too", d, 2, 4096, 3000, 256, 3u << 1);
  run("6 b2 n4096 split3 res_cap8", with(3, -1, 8), 2, 4096);
  run("7 b2 n4096 split1 cluster2", with(1, 2), 2, 4096);
  run("8a b64 n16384 split0", with(0), 64, 16384);
  run("8b b64 n16384 iters64", d, 64, 16384, 64);
  run("9 b40 n4096 split2", with(2), 40, 4096);
  {
    EmdKnobs k = with(2);
    k.plan_round = 600;
    k.plan_every = 700;
    run("10 b40 n4096 split2 plan_round600 plan_every700", k, 40, 4096);
    run("10b the same, third tiered launch refused", k, 40, 4096, 3000, 256, 1u << 4);
  }
  run("11a b64 n16384 iters555", d, 64, 16384, 555);
  run("11b b64 n16384 iters556", d, 64, 16384, 556);
  for (int b : {32, 33, 64, 65, 129}) {
    char name[32];
    std::snprintf(name, sizeof name, "12 b%d n16384", b);
    run(name, d, b, 16384);
  }
  run("13 b64 n2048", d, 64, 2048);
  {
    EmdKnobs k = d;
    k.plan_widths = widths({8, 5, 4, 4, 3, 3, 3, 2});
    run("14a b64 n16384 widths 8,5,4,4,3,3,3,2", k, 64, 16384);
    k.plan_widths = widths({8, 5, 4, 4, 3, 3, 3, 3});
    run("14b b64 n16384 widths 8,5,4,4,3,3,3,3", k, 64, 16384);
    k.plan_widths = widths({7, 5, 4, 4, 3, 3, 3, 3});
    run("14c b64 n16384 widths 7,5,4,4,3,3,3,3", k, 64, 16384);
    k.split = 2;
    run("14d b40 n4096 split2 widths 7,5,4,4,3,3,3,3 (5 slots per XCD: not read)", k, 40, 4096);
  }
  run("15a b64 n4096 split2", with(2), 64, 4096);
  run("15b b64 n4096 split5", d, 64, 4096);
  {
    EmdKnobs k = d;
    k.poll_distrust = 1;
    run("16 b2 n4096 poll_distrust", k, 2, 4096);
  }
  run("17 b2 n4096 cus0", d, 2, 4096, 3000, 0);
  return 0;
}
