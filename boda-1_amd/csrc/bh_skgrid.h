// bh_skgrid.h -- the grid of a persistent stream-K kernel (srk_kernel, conv_direct_mc, conv_wino).
//
// Host only, no HIP types: plain arithmetic, tested by a stand-alone program (tests/test_skgrid_cpu.py).
//
// An op is ntile output tiles of ipt iterations each, tile-major. A grid of G blocks shares them: logical
// block l takes iterations [l * ipb, (l + 1) * ipb), so a tile may be cut between blocks (its parts meet in
// the split-K workspace). The grid aims at ncu x blocks-per-CU resident blocks and then drops the blocks
// that would be left without work, so no block is empty: (G - 1) * ipb < total <= G * ipb.
#pragma once
#include <stdint.h>
#include <algorithm>

namespace bh {

struct sk_grid {
  uint64_t G;      // blocks
  uint32_t ipb;    // iterations per block
  uint64_t total;  // ntile * ipt (the launcher refuses 2^31 and up: the kernels count in 32 bits)
};

// splits (a configuration's tuning knob): 0 = dflt_bpc blocks per CU; 1..4 = that many, the iterations
// dealt equally (tiles cut between blocks); 5 and up = splits - 4, whole tiles per block (a persistent
// data-parallel grid: short-K ops, where cut tiles cost more than balance). Blocks per CU are clamped to
// [1, max_bpc]. ntile, ipt and ncu are at least 1.
inline sk_grid plan_sk_grid(uint64_t ntile, uint32_t ipt, uint32_t ncu, uint32_t splits, uint32_t dflt_bpc,
                            uint32_t max_bpc) {
  const bool whole = splits > 4;
  const uint32_t bpc = std::max(1u, std::min(splits ? (whole ? splits - 4 : splits) : dflt_bpc, max_bpc));
  const uint64_t total = ntile * ipt, aim = (uint64_t)ncu * bpc;
  const uint64_t ipb = whole ? (ntile + aim - 1) / aim * ipt : (total + aim - 1) / aim;
  return {(total + ipb - 1) / ipb, (uint32_t)ipb, total};
}

}  // namespace bh
