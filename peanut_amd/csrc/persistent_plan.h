// The tail plan of the persistent pointwise kernels (conv_pw256p.hip, conv_pw256wp.hip).  Plain C++17, no HIP types: a host
// program can include it (tests/c_abi/plan_host.cpp).
//
// One workgroup per CU walks a list of items.  Every workgroup gets the same number of whole tiles (n_full / G); the T mod G
// tiles left over are either
//   * cut into split_p k-ranges each (raw partial tiles + the ordered reduce, as in launch_with_tail_split) and dealt out
//     evenly.  split_p minimises the busiest workgroup's extra work: ceil(t * p / G) parts of nkt / p k-tiles plus the tile's
//     overhead per part (raw store, cursor switch); or
//   * stream-K: the tail's t * nkt k-tiles as ONE stream of units of q k-tiles, cut into equal runs for the first sk_g
//     workgroups (runs of at least four k-tiles).  Against the uniform split -- whose parts come in whole multiples per
//     workgroup (132 tail tiles cut three ways = 396 parts over 256 workgroups: two parts for most, 21 k-tiles where 16.5 would
//     do) -- every workgroup ends within one unit of the others.  A tile then has up to sk_maxp fragments; the reduce sums them
//     in workgroup order.  Only for tails of at least a quarter of a round: measured per layer (profiles/r6b), 132 tail tiles
//     of 32 k-tiles 0.502 -> 0.489 ms, 8 or 32 tail tiles level or 1 % slower (their runs are a few k-tiles long and all
//     fragments).
#pragma once
#include <stddef.h>

#include <algorithm>

namespace peanut {

// items (whole tiles + tail parts / fragments) of one workgroup: the kernels' plan tables in LDS, and their trap
constexpr int kMaxItems = 120;

struct PersistentTile {
  size_t tile_floats;        // floats of one raw partial tile
  int min_part_ktiles;       // fewest k-tiles of a uniform split's part
  double part_overhead;      // k-tile times per part
  double short_part_penalty; // ... more for a part of fewer than eight k-tiles (the previous epilogue rides on eight iterations)
  int q;                     // k-tiles per unit of the stream (2: no fragment is shorter than the two iterations the kernel needs)
  int q_idle;                // sk_q of a plan that does not stream (the kernels read it only while streaming)
  double stream_fixed;       // fixed cost of the stream: a run is two fragments on average, two raw stores / cursor switches
  bool dump_tile;            // one more scratch tile behind the partial tiles (target of a workgroup's first, empty epilogue)
};

// conv_pw_glds256wp_kernel: 256 x 256 tiles
constexpr PersistentTile kPersistent256x256{(size_t)256 * 256, 2, 1.0, 0.0, 2, 2, 2.0, true};
// conv_pw_glds256p_kernel: 256 x 128 tiles, one running sum / two-level accumulation (partial sums of two k-tiles: a fragment
// then covers the same channel groups as in an uncut tile, and the totals leave during the next item's first two iterations)
constexpr PersistentTile kPersistent256x128{(size_t)256 * 128, 4, 1.5, 2.0, 1, 1, 3.0, false};
constexpr PersistentTile kPersistent256x128Flush{(size_t)256 * 128, 4, 1.5, 2.0, 2, 1, 3.0, false};

struct PersistentPlan {
  int n_full, n_sp, split_p;               // ConvKParams fields of the same names
  int sk_units, sk_maxp, sk_g, sk_q;
  size_t part_tiles;                       // raw partial tiles the tail writes
  bool scratch_ok;                         // the partial tiles (and the dump tile) fit ws_floats
  bool fits;                               // ... and a workgroup's items fit the plan table
};

// T tiles of nkt k-tiles over G workgroups; ws_floats = 0: no scratch
inline PersistentPlan plan_persistent(int T, int G, int nkt, const PersistentTile& k, bool streamk, size_t ws_floats) {
  PersistentPlan pl{};
  const int t = T % G;
  auto uniform_cost = [&](int p) {
    const double parts = (double)(((long long)t * p + G - 1) / G);
    return parts * ((double)nkt / p + k.part_overhead + (nkt / p < 8 ? k.short_part_penalty : 0.0));
  };
  int sp = 1;
  if (t > 0) {
    double best = 1e30;
    for (int cand = 1; cand <= 16 && nkt / cand >= k.min_part_ktiles; ++cand) {
      if ((size_t)t * cand * k.tile_floats > ws_floats) break;
      const double cost = uniform_cost(cand);
      if (cost < best - 1e-9) { best = cost; sp = cand; }
    }
  }
  pl.split_p = sp;
  pl.n_sp = t * sp;
  pl.n_full = T - t;
  pl.sk_q = k.q_idle;
  const int q = k.q;
  if (t * 4 >= G && streamk && ws_floats != 0 && nkt % q == 0) {
    const int upt = nkt / q;                                        // stream units per tile
    const long long U = (long long)t * upt;
    const int Gs = (int)std::min<long long>(G, std::max<long long>(1, U * q / 4));
    const int run = (int)(U / Gs);                                  // shortest run, in units
    const int maxp = run > 0 ? (upt + run - 1) / run + 1 : 0;
    const double cost_stream = (double)((U + Gs - 1) / Gs) * q + k.stream_fixed;
    if (run * q >= 4 && (size_t)t * maxp * k.tile_floats <= ws_floats && cost_stream < uniform_cost(sp) - 0.5) {
      pl.sk_units = (int)U; pl.sk_maxp = maxp; pl.sk_g = Gs; pl.sk_q = q;
      pl.n_sp = 0; pl.split_p = 1;
    }
  }
  pl.part_tiles = pl.sk_units > 0 ? (size_t)t * pl.sk_maxp : (size_t)pl.n_sp;
  pl.scratch_ok = (pl.part_tiles + (k.dump_tile ? 1 : 0)) * k.tile_floats <= ws_floats;
  // whole tiles + the workgroup's tail parts (or <= 3 fragments) + slack
  pl.fits = pl.scratch_ok && pl.n_full / G + (pl.n_sp + G - 1) / G + 4 <= kMaxItems;
  return pl;
}

}  // namespace peanut
