// Host program of tests/test_persistent_plan_cpu.py: the tail plan of the persistent pointwise kernels
// (peanut_amd/csrc/persistent_plan.h, plain C++17) over the sweep of tests/golden/persistent_plans.json, one row per line:
//   kernel T G nkt ws_floats streamk flush n_full n_sp split_p sk_units sk_maxp sk_g sk_q status part_tiles tile_floats dump
// status: "fits"; "declined" (the route takes the next kernel); "error" (256 x 128: the launcher fails, split-K scratch too small).
#include <cstdio>

#include "persistent_plan.h"

int main() {
  using namespace peanut;
  const int Ts[] = {1, 7, 8, 255, 256, 257, 388, 900, 1800, 3600, 65536};
  const int Gs[] = {8, 64, 256, 304};
  const int nkts[] = {2, 4, 8, 16, 17, 32, 64};
  const size_t kScratch = (size_t)48 << 20;      // kSplitKScratchFloats (common.h)
  std::printf("kMaxItems %d\n", kMaxItems);
  for (int kern = 0; kern < 3; ++kern) {         // 256 x 256, 256 x 128 with one running sum, 256 x 128 with partial sums of two k-tiles
    const PersistentTile& k = kern == 0 ? kPersistent256x256 : (kern == 1 ? kPersistent256x128 : kPersistent256x128Flush);
    const size_t wss[] = {0, k.tile_floats, 64 * k.tile_floats, kScratch};
    for (int T : Ts) for (int G : Gs) for (int nkt : nkts) for (size_t ws : wss) for (int sk = 0; sk < 2; ++sk) {
      const PersistentPlan p = plan_persistent(T, G, nkt, k, sk != 0, ws);
      const char* status = p.fits ? "fits" : ((kern != 0 && !p.scratch_ok) ? "error" : "declined");
      std::printf("%s %d %d %d %zu %d %d %d %d %d %d %d %d %d %s %zu %zu %d\n", kern == 0 ? "256x256p" : "256x128p", T, G, nkt, ws, sk,
                  kern == 2 ? 2 : 0, p.n_full, p.n_sp, p.split_p, p.sk_units, p.sk_maxp, p.sk_g, p.sk_q, status, p.part_tiles,
                  k.tile_floats, k.dump_tile ? 1 : 0);
    }
  }
  return 0;
}
