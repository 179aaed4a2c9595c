// The planner-side map bookkeeping of the reference's Agent_Helper._plan (nav/agent/agent_helper.py:272-315) on the device: the
// line the agent walked since the last step drawn into visited_vis (vu.draw_line, nav/agent/utils/visualization.py:19-24) and the
// cells in front of a bump set in collision_map.  Both maps are read by the goal selection (goal.hip) and the short-term goal
// (stg.hip); this file is the only writer the product has.
//
// The reference does it on the host on two float64 maps.  Here the maps are the uint8 [full_w, full_h] device tensors the readers
// already take, and the whole update is ONE launch for 1..PEANUT_PLAN_MAX_BATCH episodes: grid (1, E), one thread per (line point,
// corner of its 2 x 2 block) and one per collision cell, each a plain byte store of the value 1.  Several threads may store the same
// 1 into one byte; nothing is read, so there is no order to keep and no atomic.
//
// Everything that involves a float stays on the host.  The 26 line points are computed there in double, operation by operation as
// NumPy does (peanut_plan_line); the collision cells come from the caller as integers (the reference forms them with np.cos / np.sin /
// np.deg2rad and an int() truncation: the caller's NumPy owns their last bit).  Points and cells travel by value in the kernel
// arguments: a point as 12 + 12 bits, a cell as 16 + 16 bits, 224 bytes per episode.
#include <cmath>
#include <string>

#include "../../include/peanut_hip.h"
#include "common.h"

namespace peanut {

namespace {

constexpr int PL_POINTS = PEANUT_PLAN_LINE_POINTS;                    // 26
constexpr int PL_POINT_THREADS = 4 * PL_POINTS;                       // a 2 x 2 block per point
constexpr int PL_THREADS = 192;                                       // >= 104 + PEANUT_PLAN_MAX_CELLS
constexpr int PL_POINT_WORDS = (PL_POINTS * 24 + 31) / 32;            // 20
constexpr int PL_MAX_M = 4096, PL_MAX_FULL = 65536;                   // what the packing holds
static_assert(PL_POINT_THREADS + PEANUT_PLAN_MAX_CELLS <= PL_THREADS, "one thread per store");

struct PlanMarkP {
  unsigned char* visited;                    // [full_w, full_h]
  unsigned char* collision;                  // [full_w, full_h]
  int gx1, gy1, n_cells;
  int reserved;
  unsigned points[PL_POINT_WORDS];           // point k: bits [24 k, 24 k + 12) = x, the next 12 = y (window coordinates)
  unsigned cells[PEANUT_PLAN_MAX_CELLS];     // r | c << 16 (full-map coordinates)
};
struct PlanMarkBatchArgs {
  PlanMarkP p[PEANUT_PLAN_MAX_BATCH];
};
static_assert(sizeof(PlanMarkBatchArgs) <= 3840, "the argument block must stay below 4 KiB with the hidden arguments");

__global__ __launch_bounds__(PL_THREADS) void plan_mark_kernel(const PlanMarkBatchArgs A, int full_h) {
  const PlanMarkP& p = A.p[blockIdx.y];
  const int t = threadIdx.x;
  if (t < PL_POINT_THREADS) {
    const int k = t >> 2, bit = 24 * k, w = bit >> 5, sh = bit & 31;
    const unsigned long long two = (unsigned long long)p.points[w] | ((unsigned long long)p.points[w + 1 < PL_POINT_WORDS ? w + 1 : w] << 32);
    const unsigned v = (unsigned)(two >> sh);
    const int x = (int)(v & 0xfffu), y = (int)((v >> 12) & 0xfffu);
    // mat[x - 1:x + 1, y - 1:y + 1] = 1 on the m x m view: rows x - 1 and x, EMPTY when x == 0 (`[-1:1]`, m >= 2); the same for y
    if (x >= 1 && y >= 1) {
      const int r = p.gx1 + x - 1 + ((t >> 1) & 1), c = p.gy1 + y - 1 + (t & 1);
      p.visited[(size_t)r * full_h + c] = 1;
    }
  } else if (t - PL_POINT_THREADS < p.n_cells) {
    const unsigned v = p.cells[t - PL_POINT_THREADS];
    p.collision[(size_t)(v & 0xffffu) * full_h + (v >> 16)] = 1;
  }
}

void plan_line(const int last_start[2], const int start[2], int pts[PL_POINTS][2]) {
  for (int i = 0; i < PL_POINTS; ++i)
    for (int a = 0; a < 2; ++a) {
      // start[a] + (end[a] - start[a]) * i / steps with Python ints: an integer product, one true division, one add; np.rint
      const long long prod = (long long)(start[a] - last_start[a]) * i;
      const double q = (double)prod / 25.0;
      pts[i][a] = (int)std::nearbyint((double)last_start[a] + q);        // the default rounding mode: to nearest, ties to even
    }
}

// the checks of one episode and its packed arguments; nothing is enqueued before every episode has passed
int plan_mark_params(PlanMarkP& p, const peanut_plan_maps_t* maps, const peanut_plan_mark_t* ep) {
  if (!ep->visited_vis || !ep->collision_map) return fail(PEANUT_EINVAL, "peanut_plan_mark: null map");
  const int gx1 = ep->lmb[0], gx2 = ep->lmb[1], gy1 = ep->lmb[2], gy2 = ep->lmb[3];
  const int m = gx2 - gx1;
  if (m < 2 || m > PL_MAX_M) return fail(PEANUT_EINVAL, "peanut_plan_mark: the window must be 2..4096 cells wide");
  if (gy2 - gy1 != m || gx1 < 0 || gy1 < 0 || gx2 > maps->full_w || gy2 > maps->full_h)
    return fail(PEANUT_EINVAL, "peanut_plan_mark: lmb is not an m x m window inside the full map");
  for (int a = 0; a < 2; ++a)
    if (ep->last_start[a] < 0 || ep->last_start[a] >= m || ep->start[a] < 0 || ep->start[a] >= m)
      return fail(PEANUT_EINVAL, "peanut_plan_mark: start and last_start must lie in [0, m)");
  if (ep->n_cells < 0 || ep->n_cells > PEANUT_PLAN_MAX_CELLS) return fail(PEANUT_EINVAL, "peanut_plan_mark: n_cells must be 0..PEANUT_PLAN_MAX_CELLS");
  p = PlanMarkP{};
  p.visited = ep->visited_vis;
  p.collision = ep->collision_map;
  p.gx1 = gx1; p.gy1 = gy1; p.n_cells = ep->n_cells;
  for (int k = 0; k < ep->n_cells; ++k) {
    const int r = ep->cells_rc[k][0], c = ep->cells_rc[k][1];
    if (r < 0 || r >= maps->full_w || c < 0 || c >= maps->full_h) return fail(PEANUT_EINVAL, "peanut_plan_mark: a collision cell lies outside the map");
    p.cells[k] = (unsigned)r | ((unsigned)c << 16);
  }
  int pts[PL_POINTS][2];
  plan_line(ep->last_start, ep->start, pts);
  for (int k = 0; k < PL_POINTS; ++k) {
    if (pts[k][0] < 0 || pts[k][0] >= m || pts[k][1] < 0 || pts[k][1] >= m)       // (cannot happen: a point lies between its ends)
      return fail(PEANUT_EINVAL, "peanut_plan_mark: a line point left the window");
    const unsigned long long v = ((unsigned long long)pts[k][0] | ((unsigned long long)pts[k][1] << 12)) << ((24 * k) & 31);
    const int w = (24 * k) >> 5;
    p.points[w] |= (unsigned)v;
    if (v >> 32) p.points[w + 1] |= (unsigned)(v >> 32);
  }
  return 0;
}

int plan_mark_launch(const peanut_plan_maps_t* maps, int E, const peanut_plan_mark_t* eps, const char* who) {
  if (!maps || !eps) return fail(PEANUT_EINVAL, std::string(who) + ": null argument");
  if (E < 1 || E > PEANUT_PLAN_MAX_BATCH) return fail(PEANUT_EINVAL, std::string(who) + ": E must be 1..PEANUT_PLAN_MAX_BATCH");
  if (maps->full_w < 2 || maps->full_h < 2 || maps->full_w > PL_MAX_FULL || maps->full_h > PL_MAX_FULL)
    return fail(PEANUT_EINVAL, std::string(who) + ": the full map must be 2..65536 cells on each side");
  PlanMarkBatchArgs A{};
  const uintptr_t n = (uintptr_t)maps->full_w * (uintptr_t)maps->full_h;
  for (int e = 0; e < E; ++e) {
    if (int rc = plan_mark_params(A.p[e], maps, eps + e)) return rc;
    // [map, map + full_w * full_h) of no two of the 2 E maps may meet (an episode's own two maps included)
    const uintptr_t mine[2] = {(uintptr_t)eps[e].visited_vis, (uintptr_t)eps[e].collision_map};
    if (mine[0] < mine[1] + n && mine[1] < mine[0] + n) return fail(PEANUT_EINVAL, std::string(who) + ": an episode's two maps overlap");
    for (int o = 0; o < e; ++o) {
      const uintptr_t other[2] = {(uintptr_t)eps[o].visited_vis, (uintptr_t)eps[o].collision_map};
      for (uintptr_t a : mine)
        for (uintptr_t b : other)
          if (a < b + n && b < a + n) return fail(PEANUT_EINVAL, std::string(who) + ": two episodes name the same map");
    }
  }
  hipLaunchKernelGGL(plan_mark_kernel, dim3(1, E), dim3(PL_THREADS), 0, (hipStream_t)maps->stream, A, maps->full_h);
  hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : fail(PEANUT_EHIP, std::string(who) + ": " + hipGetErrorString(err));
}

}  // namespace

}  // namespace peanut

using namespace peanut;

extern "C" int peanut_plan_line(const int last_start[2], const int start[2], int points_out[PEANUT_PLAN_LINE_POINTS][2]) {
  if (!last_start || !start || !points_out) return fail(PEANUT_EINVAL, "peanut_plan_line: null argument");
  plan_line(last_start, start, points_out);
  return 0;
}

extern "C" int peanut_plan_mark(const peanut_plan_maps_t* maps, const peanut_plan_mark_t* episode) {
  return plan_mark_launch(maps, 1, episode, "peanut_plan_mark");
}

extern "C" int peanut_plan_mark_batch(const peanut_plan_maps_t* maps, int E, const peanut_plan_mark_t* episodes) {
  return plan_mark_launch(maps, E, episodes, "peanut_plan_mark_batch");
}
