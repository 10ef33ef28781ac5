// Stand-alone check of the persistent stream-K grid planner (boda-1_amd/csrc/bh_skgrid.h), built with
// AddressSanitizer + UBSan by tests/test_skgrid_cpu.py. Prints "case <name> ok" per case; any failed
// expectation prints the line and makes the exit status 1.
#include <stdio.h>
#include "bh_skgrid.h"

static int g_fail = 0;
#define EXPECT(x)                                              \
  do {                                                         \
    if (!(x)) {                                                \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);    \
      g_fail = 1;                                              \
    }                                                          \
  } while (0)

// the grids the launchers planned before they shared the planner, recorded from their formula
static void rows() {
  struct row {
    uint64_t ntile;
    uint32_t ipt, ncu, splits, dflt_bpc, max_bpc;
    uint64_t G;
    uint32_t ipb;
    uint64_t total;
  };
  const row R[] = {
      {300, 9, 256, 0, 2, 4, 450, 6, 2700},      {300, 9, 256, 3, 2, 2, 450, 6, 2700},
      {300, 9, 256, 6, 2, 4, 300, 9, 2700},      {1000, 4, 256, 5, 1, 4, 250, 16, 4000},
      {7, 100, 256, 1, 1, 4, 234, 3, 700},       {1, 3, 256, 0, 1, 1, 3, 1, 3},
      {513, 1, 256, 8, 2, 3, 513, 1, 513},       {2048, 16, 256, 4, 2, 4, 1024, 32, 32768},
  };
  for (const row &r : R) {
    const bh::sk_grid g = bh::plan_sk_grid(r.ntile, r.ipt, r.ncu, r.splits, r.dflt_bpc, r.max_bpc);
    if (g.G != r.G || g.ipb != r.ipb || g.total != r.total)
      printf("row %llu %u %u %u %u %u: got %llu %u %llu\n", (unsigned long long)r.ntile, r.ipt, r.ncu, r.splits,
             r.dflt_bpc, r.max_bpc, (unsigned long long)g.G, g.ipb, (unsigned long long)g.total);
    EXPECT(g.G == r.G && g.ipb == r.ipb && g.total == r.total);
  }
  printf("case rows ok\n");
}

// no block is empty, none is missing, and the whole-tile modes cut no tile
static void invariants() {
  const uint64_t ntiles[] = {1, 2, 7, 255, 256, 257, 300, 513, 2048, 100000};
  const uint32_t ipts[] = {1, 2, 3, 9, 16, 100}, ncus[] = {1, 8, 256, 304};
  long n = 0;
  for (uint64_t ntile : ntiles)
    for (uint32_t ipt : ipts)
      for (uint32_t ncu : ncus)
        for (uint32_t splits = 0; splits <= 9; ++splits)
          for (uint32_t dflt = 1; dflt <= 2; ++dflt)
            for (uint32_t cap = 1; cap <= 4; ++cap) {
              const bh::sk_grid g = bh::plan_sk_grid(ntile, ipt, ncu, splits, dflt, cap);
              EXPECT(g.total == ntile * ipt && g.ipb >= 1 && g.G >= 1);
              EXPECT(g.G * g.ipb >= g.total);
              EXPECT((g.G - 1) * g.ipb < g.total);
              if (splits > 4) EXPECT(g.ipb % ipt == 0);
              // never more blocks than the CUs hold at the capped blocks per CU
              EXPECT(g.G <= (uint64_t)ncu * cap);
              ++n;
            }
  printf("swept %ld grids\n", n);
  printf("case invariants ok\n");
}

// the knob's readings: 0 is the default, 1..4 and 5..8 name the same blocks per CU, the cap holds
static void knob() {
  const uint64_t ntile = 5000;
  const uint32_t ipt = 7, ncu = 256;
  for (uint32_t b = 1; b <= 4; ++b) {
    const bh::sk_grid even = bh::plan_sk_grid(ntile, ipt, ncu, b, 1, 4), dflt = bh::plan_sk_grid(ntile, ipt, ncu, 0, b, 4);
    EXPECT(even.G == dflt.G && even.ipb == dflt.ipb);
    EXPECT(even.ipb == (ntile * ipt + ncu * b - 1) / (ncu * b));
    const bh::sk_grid whole = bh::plan_sk_grid(ntile, ipt, ncu, b + 4, 1, 4);
    EXPECT(whole.ipb == (ntile + ncu * b - 1) / (ncu * b) * ipt);
    const bh::sk_grid capped = bh::plan_sk_grid(ntile, ipt, ncu, b, 1, 2), at2 = bh::plan_sk_grid(ntile, ipt, ncu, b < 2 ? b : 2, 1, 4);
    EXPECT(capped.G == at2.G && capped.ipb == at2.ipb);
  }
  // a zero default or cap still leaves one block per CU
  const bh::sk_grid z = bh::plan_sk_grid(ntile, ipt, ncu, 0, 0, 0), one = bh::plan_sk_grid(ntile, ipt, ncu, 1, 1, 4);
  EXPECT(z.G == one.G && z.ipb == one.ipb);
  printf("case knob ok\n");
}

int main() {
  rows();
  invariants();
  knob();
  if (!g_fail) printf("skgrid check ok\n");
  return g_fail;
}
