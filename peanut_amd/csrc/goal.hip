// Long-term goal selection on the device: the reference's
// Agent_State.update_global_goal (nav/agent/agent_state.py:376-415) and the geodesic distance transform of
// FMMPlanner.set_goal / set_multi_goal (nav/agent/utils/fmm_planner.py:55-75).
//
// The reference computes the geodesic field with scikit-fmm (`skfmm.distance`, heap-ordered fast marching, second
// order) on the host: ~0.2 s per call on a 960x960 map, the largest CPU cost per step once stages 1-3 run on the
// GPU.  A heap is inherently serial.  Here the same discretisation (second-order upwind differences with the
// first-order fallback, masked cells excluded from every stencil; oracle/fmm_ref.c states the update rule that is
// mirrored operation by operation, in double) is solved by relaxation, arranged so that every stage provably ends:
//
//   * tiles: the map is cut into 32x32 tiles; a workgroup stages a tile plus a 2-cell halo in LDS and relaxes it until nothing
//     in the tile changes -- since round 5 block-wise (fmm_round_blocked_kernel): each of the 16 waves owns an 8 x 8 block, keeps
//     a private copy of it with its two-cell ring and iterates it to convergence between two workgroup barriers (Jacobi inside
//     the wave, which needs no barrier), then publishes it; the older form (fmm_round_kernel, option fmm_blocked = 0) sweeps
//     the whole tile once per barrier pair.  A tile that changed wakes its four neighbours for the next round (the stencil is
//     axis-aligned: no diagonal dependency); rounds are plain launches over the tile grid in which sleeping tiles exit at
//     once; the host reads one counter every few rounds.  Only a ring of tiles is awake in a round, so a round costs the
//     LATENCY of its slowest tile: the number of iterations the front needs to cross it times the dependent instruction
//     chain of one update (profiles/r8/README.md), which is what the blocked form and update_cell_local_fast shorten;
//   * stage A, first order: u <- min(u, update(u)) from +inf.  Monotone, hence convergent, to the unique first-order
//     field u1 (the classic fast iterative method);
//   * stage B, second order, on a FIXED dependency graph: a neighbour may feed a cell only if it precedes the cell in
//     a given ordering field `ord` (stage A's u1 at first).  The graph is acyclic, so a plain fixed-point sweep
//     u <- update(u) settles cell after cell in that order -- no "keep the smaller" is needed (the second-order term
//     is not monotone in its second neighbour: keeping minima would freeze transients) and none of the feedback that
//     makes an unrestricted second-order relaxation oscillate (two cells each taking the other for its upwind
//     neighbour) can occur;
//   * stage B is repeated with `ord` = its own result, warm-started (later passes only touch the cells whose order
//     moved).  Iterated until nothing changes (5-6 passes) the result is the self-consistent second-order field, 0.14
//     cell from the heap-ordered march on maze maps (reached within six passes, the cap),
//     which bounds the cost: every pass is a front propagation across the map, ~1.5 ms at 960 x 960.
//
// Difference to the heap-ordered march: when the two-axis root falls BELOW the value of the later of its two
// neighbours (possible with second-order terms next to walls), scikit-fmm's march keeps it -- the neighbour was
// already frozen -- while the relaxation keeps the causal one-axis root.  Measured on maze maps: <= 0.14 cell
// max-abs, far from walls identical to rounding; tests hold the field to <= 0.5 cell of the oracle and the selected
// goal cell to equality.
//
// The rest of update_global_goal is fused around it: obstacle dilation by the collision disk + collision / visited
// overrides -> traversible map (:382-386), the fill (:392-393: the cells equal to the field's maximum become +inf -- the
// unreached ones, or the farthest reached ones when every cell was reached), exp(-d / temperature) weights with the "stuck:
// keep the last weights" rule (:395-399; their sum is reduced in a fixed order, so the rule decides the same on every run),
// value = target_pred * weights and its argmax with np.argmax's semantics (first occurrence; the first NaN wins) (:401-413).
//
// The field needs the map, not the prediction: peanut_goal_select_begin puts the traversible map, the initialisation and the first
// batch of relaxation rounds on a stream of the handle at once; the forward the caller enqueues next (Agent_State.update_state:
// update_prediction then update_global_goal) runs beside them, peanut_goal_select continues the solve on that stream, and the
// caller's stream joins before the weights are formed.
//
// Several episodes (Agent_State_Group: E episodes per GPU in lock-step select their goals on the same steps): a round wakes a ring of
// tiles and costs the latency of one, so E solves in a row leave most CUs idle E times over and synchronise E times per stage.
// peanut_goal_select_batch runs up to PEANUT_GOAL_MAX_BATCH episodes in the launches and synchronisations of ONE solve: a round is
// one launch over (tiles, E), a check one read-back of the [E][rounds] counters.  Every episode keeps its own handle and sees the
// rounds of its own solve with rounds that wake none of its tiles in between -- its results are the bits of peanut_goal_select.
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "goal_internal.h"
#include "net_common.h"

#pragma clang fp contract(off)

namespace peanut {
namespace {

constexpr int TILE = 32, HALO = 2, LT = TILE + 2 * HALO;   // 36
constexpr int MAX_SWEEPS = 96;                             // per round and tile (a front crosses a tile in <= 64)
constexpr int ROUNDS_PER_CHECK = 8, MAX_ROUNDS_PER_CHECK = 96;
constexpr int MAX_ORDER_PASSES = 24;    // default of option fmm_max_passes: a ceiling, the passes end at their fixed point (round 5; a cap of six left the deployed 960 x 960 map unconverged); measured distance to the heap-ordered march: 3 passes 0.39 / 0.70 cell (maze / cluttered map), 4 passes 0.14 / 0.47, fixed point (5-6) 0.14 / 0.03

enum : unsigned char { ST_MASKED = 0, ST_FREE = 1, ST_SEED = 2 };

// Every kernel below exists twice: for one episode, and for up to GB episodes in one launch (peanut_goal_select_batch: the
// episode is blockIdx.y -- blockIdx.z for the two-dimensional traversible grid -- and the per-episode pointers and scalars travel
// by value in a struct of GB slots).  Both are thin wrappers around ONE __device__ body, so an expression two kernels must agree on
// bit for bit lives in one function.
constexpr int GB = PEANUT_GOAL_MAX_BATCH;
struct TravBatchArgs {
  const float* obst[GB];
  const unsigned char *col[GB], *vis[GB];
  unsigned char* trav[GB];
};
struct FieldBatchArgs {
  double* dist[GB];
  double* ord[GB];
  unsigned char* state[GB];
  unsigned char* active[GB];      // four flag arrays of tiles_x * tiles_y bytes each (field_preamble)
  int seed_r[GB], seed_c[GB];
  unsigned int done;              // bit e: episode e takes no part in this launch (its passes ended, its stage has settled, or the caller left it out)
};
// the batched field on given masks (fmm_distance_masks_batch): what peanut_fmm_distance(g, trav, goal_mask, -1, -1, 1, out) takes, per episode
struct MaskBatchArgs {
  const unsigned char *trav[GB], *seed[GB];
  unsigned long long* max_bits[GB];      // slot 0 of the episode's own maxbits, as in the single call
  double* out[GB];
};

// ---- traversible map: ~dilate(rint(obstacle), disk(rad)), collision -> 0, visited -> 1  (agent_state.py:382-386) ----
// A workgroup covers 32 x 8 cells.  The obstacle bits of its rows (8 + 2 rad of them, 32 + 2 rad columns wide: one 64-bit word per
// row while rad <= 16) are formed once with a ballot per row; a cell is blocked when any row of its disk has an obstacle bit under
// that row's chord -- 2 rad + 1 AND-tests instead of (2 rad + 1)^2 loads (85 -> ~12 us on the 960 x 960 map).
constexpr int TRAV_MAX_RAD = 16;
__device__ __forceinline__ void goal_trav_body(const float* __restrict__ obst, const unsigned char* __restrict__ collision,
                                               const unsigned char* __restrict__ visited, int H, int W, int rad,
                                               unsigned char* __restrict__ trav) {
  __shared__ unsigned long long rowbits[8 + 2 * TRAV_MAX_RAD];
  __shared__ int chord[2 * TRAV_MAX_RAD + 1];      // half-width of the disk at row offset dy
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 8;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int span = 32 + 2 * rad;                    // <= 64
  for (int rr = wave; rr < 8 + 2 * rad; rr += 4) {
    const int r = r0 - rad + rr, c = c0 - rad + lane;
    const bool ob = lane < span && r >= 0 && r < H && c >= 0 && c < W && rintf(obst[(size_t)r * W + c]) != 0.f;
    const unsigned long long m = __ballot(ob);
    if (lane == 0) rowbits[rr] = m;
  }
  if (threadIdx.x <= 2 * rad) {
    const int dy = (int)threadIdx.x - rad;
    int w = 0;
    while ((w + 1) * (w + 1) + dy * dy <= rad * rad) ++w;
    chord[threadIdx.x] = w;
  }
  __syncthreads();
  const int lc = threadIdx.x & 31, lr = threadIdx.x >> 5;
  const int c = c0 + lc, r = r0 + lr;
  if (r >= H || c >= W) return;
  bool blocked = false;
  for (int dy = -rad; dy <= rad; ++dy) {
    const int w = chord[dy + rad];
    // bits lc + rad - w .. lc + rad + w of the row (bit b = column c0 - rad + b)
    const unsigned long long mask = ((w + w + 1 >= 64) ? ~0ull : ((1ull << (w + w + 1)) - 1ull)) << (lc + rad - w);
    blocked = blocked || (rowbits[lr + rad + dy] & mask) != 0ull;
  }
  unsigned char t = blocked ? 0 : 1;
  const size_t i = (size_t)r * W + c;
  if (collision && collision[i] == 1) t = 0;
  if (visited && visited[i] == 1) t = 1;
  trav[i] = t;
}
__global__ __launch_bounds__(256) void goal_trav_kernel(const float* __restrict__ obst, const unsigned char* __restrict__ collision,
                                                        const unsigned char* __restrict__ visited, int H, int W, int rad,
                                                        unsigned char* __restrict__ trav) {
  goal_trav_body(obst, collision, visited, H, W, rad, trav);
}
__global__ __launch_bounds__(256) void goal_trav_batch_kernel(TravBatchArgs a, int H, int W, int rad) {
  const int e = blockIdx.z;
  goal_trav_body(a.obst[e], a.col[e], a.vis[e], H, W, rad, a.trav[e]);
}
// any radius (the footprint test cell by cell): used beyond TRAV_MAX_RAD
__device__ __forceinline__ void goal_trav_wide_body(const float* __restrict__ obst, const unsigned char* __restrict__ collision,
                                                    const unsigned char* __restrict__ visited, int H, int W, int rad,
                                                    unsigned char* __restrict__ trav) {
  const int c = blockIdx.x * 32 + (threadIdx.x & 31), r = blockIdx.y * 8 + (threadIdx.x >> 5);
  if (r >= H || c >= W) return;
  bool blocked = false;
  for (int dy = -rad; dy <= rad && !blocked; ++dy) {
    const int rr = r + dy;
    if (rr < 0 || rr >= H) continue;
    for (int dx = -rad; dx <= rad; ++dx) {
      if (dx * dx + dy * dy > rad * rad) continue;
      const int cc = c + dx;
      if (cc < 0 || cc >= W) continue;
      if (rintf(obst[(size_t)rr * W + cc]) != 0.f) { blocked = true; break; }
    }
  }
  unsigned char t = blocked ? 0 : 1;
  const size_t i = (size_t)r * W + c;
  if (collision && collision[i] == 1) t = 0;
  if (visited && visited[i] == 1) t = 1;
  trav[i] = t;
}

__global__ __launch_bounds__(256) void goal_trav_wide_kernel(const float* __restrict__ obst, const unsigned char* __restrict__ collision,
                                                             const unsigned char* __restrict__ visited, int H, int W, int rad,
                                                             unsigned char* __restrict__ trav) {
  goal_trav_wide_body(obst, collision, visited, H, W, rad, trav);
}
__global__ __launch_bounds__(256) void goal_trav_wide_batch_kernel(TravBatchArgs a, int H, int W, int rad) {
  const int e = blockIdx.z;
  goal_trav_wide_body(a.obst[e], a.col[e], a.vis[e], H, W, rad, a.trav[e]);
}

// state / distance initialisation: masked where not traversible, seeds (one cell and/or a mask) at distance 0.  `active`: the seeds'
// tiles are flagged there; `active2` (optional): and there -- the batched form flags the seed-tile array and the first round's input
// in one launch, where the single solve copies one to the other.
__device__ __forceinline__ void fmm_init_body(const unsigned char* __restrict__ trav, const unsigned char* __restrict__ seed_mask,
                                              int seed_r, int seed_c, int H, int W, unsigned char* __restrict__ state,
                                              double* __restrict__ dist, unsigned char* __restrict__ active,
                                              unsigned char* __restrict__ active2, int tiles_x) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= H * W) return;
  const int r = i / W, c = i - r * W;
  const bool seed = (r == seed_r && c == seed_c) || (seed_mask && seed_mask[i] == 1);
  state[i] = seed ? ST_SEED : (trav[i] ? ST_FREE : ST_MASKED);
  dist[i] = seed ? 0.0 : INFINITY;
  if (seed) {
    active[(r / TILE) * tiles_x + (c / TILE)] = 1;
    if (active2) active2[(r / TILE) * tiles_x + (c / TILE)] = 1;
  }
}
__global__ __launch_bounds__(256) void fmm_init_kernel(const unsigned char* __restrict__ trav, const unsigned char* __restrict__ seed_mask,
                                                       int seed_r, int seed_c, int H, int W, unsigned char* __restrict__ state,
                                                       double* __restrict__ dist, unsigned char* __restrict__ active, int tiles_x) {
  fmm_init_body(trav, seed_mask, seed_r, seed_c, H, W, state, dist, active, nullptr, tiles_x);
}
// all four flag arrays of every episode to zero: the batched solve's memset (one launch instead of E)
__global__ __launch_bounds__(256) void fmm_flags_clear_batch_kernel(FieldBatchArgs a, int nflags) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < nflags) a.active[blockIdx.y][i] = 0;
}
__global__ __launch_bounds__(256) void fmm_init_batch_kernel(FieldBatchArgs a, TravBatchArgs t, int H, int W, int tiles_x, int nt) {
  const int e = blockIdx.y;
  unsigned char* act = a.active[e];
  fmm_init_body(t.trav[e], nullptr, a.seed_r[e], a.seed_c[e], H, W, a.state[e], a.dist[e], act + 3 * (size_t)nt, act, tiles_x);
}
// the same with a seed MASK per episode (no seed cell) on maps the caller gives; also zeroes the slot the fill's maximum is formed in
__global__ __launch_bounds__(256) void fmm_init_mask_batch_kernel(FieldBatchArgs a, MaskBatchArgs m, int H, int W, int tiles_x, int nt) {
  const int e = blockIdx.y;
  if ((a.done >> e) & 1u) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) *m.max_bits[e] = 0ull;
  unsigned char* act = a.active[e];
  fmm_init_body(m.trav[e], m.seed[e], -1, -1, H, W, a.state[e], a.dist[e], act + 3 * (size_t)nt, act, tiles_x);
}

// one axis of distanceMarcher::updatePointOrderTwo.  m1/m2 = the values one and two steps towards smaller indices,
// p1/p2 towards larger ones; INFINITY = masked / outside / not reached / not allowed to feed this cell.
struct AxisTerm { double a, b, c, v1; };
__device__ __forceinline__ AxisTerm axis_term(double m1, double m2, double p1, double p2) {
  AxisTerm t{0.0, 0.0, 0.0, INFINITY};
  double v1 = INFINITY, v2 = INFINITY;
  // j = -1 first; j = +1 only when strictly closer; the second neighbour when it is not farther than the first (<=).
  // The library's loop leaves a v2 found in the j = -1 direction in place when j = +1 then supplies the closer v1 without
  // a qualifying second neighbour (oracle/fmm_ref.c keeps that); here v2 always belongs to v1's own side: the mixed pair
  // (v1 from one side, v2 from the other) only arises where two fronts meet, is not an upwind difference, and with it the
  // ordering passes of this solver stop reaching a fixed point (measured: profiles/r3f)
  if (m1 < v1) { v1 = m1; v2 = (m2 <= v1) ? m2 : INFINITY; }
  if (p1 < v1) { v1 = p1; v2 = (p2 <= v1) ? p2 : INFINITY; }
  t.v1 = v1;
  if (v2 < INFINITY) {
    const double aa = 9.0 / 4.0, tp = (1.0 / 3.0) * (4.0 * v1 - v2);
    t.a = aa; t.b = -2.0 * aa * tp; t.c = aa * tp * tp;
  } else if (v1 < INFINITY) {
    t.a = 1.0; t.b = -2.0 * v1; t.c = v1 * v1;
  }
  return t;
}
__device__ __forceinline__ double solve_root(double a, double b, double c) {
  c -= 1.0;
  const double det = b * b - 4.0 * a * c;
  return det >= 0.0 ? (-b + sqrt(det)) / 2.0 / a : -1.0;
}
// Upwind selection: the axis with the smaller neighbour alone first; the other axis joins only when its neighbour
// lies strictly below that one-axis value (it is then upwind of the cell) and the joint root stays above it.
__device__ __forceinline__ double update_cell(const AxisTerm& y, const AxisTerm& x) {
  const bool hy = y.v1 < INFINITY, hx = x.v1 < INFINITY;
  if (!hy && !hx) return INFINITY;
  const bool y_first = hy && (!hx || y.v1 <= x.v1);
  const AxisTerm& s = y_first ? y : x;
  const AxisTerm& o = y_first ? x : y;
  const double u1 = solve_root(s.a, s.b, s.c);
  if (o.v1 < u1) {
    const double u2 = solve_root(s.a + o.a, s.b + o.b, s.c + o.c);
    if (u2 > o.v1) return u2;
  }
  return u1;
}

// The same update with the quadratic solved RELATIVE to the smaller upwind value, in single precision: the unknown
// is u - base with base = min(v1_y, v1_x), every input a difference of neighbouring values (O(1) cells), so float
// carries ~1e-7 cell per update where the double form needs its 15 digits only to cancel the common offset (~10^2..10^3
// cells) out of b^2 - 4ac.  A fraction of the double instruction count (v_sqrt_f32 instead of a double square-root
// sequence); the result is added back onto `base` in double.
struct AxisPick { double v1, v2; };      // nearest upwind value and the one behind it (INFINITY: none)
__device__ __forceinline__ AxisPick axis_pick(double m1, double m2, double p1, double p2) {
  AxisPick t{INFINITY, INFINITY};
  if (m1 < t.v1) { t.v1 = m1; t.v2 = (m2 <= t.v1) ? m2 : INFINITY; }      // as axis_term
  if (p1 < t.v1) { t.v1 = p1; t.v2 = (p2 <= t.v1) ? p2 : INFINITY; }
  return t;
}
__device__ __forceinline__ double update_cell_local(const AxisPick& y, const AxisPick& x) {
  const bool hy = y.v1 < INFINITY, hx = x.v1 < INFINITY;
  if (!hy && !hx) return INFINITY;
  const bool y_first = hy && (!hx || y.v1 <= x.v1);
  const AxisPick& s = y_first ? y : x;
  const AxisPick& o = y_first ? x : y;
  const double base = s.v1;
  const bool s2 = s.v2 < INFINITY;
  const float as = s2 ? 2.25f : 1.0f;
  const float ts = s2 ? (float)(s.v1 - s.v2) * (1.0f / 3.0f) : 0.0f;      // (4 v1 - v2) / 3 - base
  float r = ts + (s2 ? (2.0f / 3.0f) : 1.0f);                             // one-axis root: t + 1 / sqrt(a)
  if (o.v1 < INFINITY) {
    const float ov = (float)(o.v1 - base);
    if (ov < r) {
      const bool o2 = o.v2 < INFINITY;
      const float ao = o2 ? 2.25f : 1.0f;
      const float to = o2 ? ov + (float)(o.v1 - o.v2) * (1.0f / 3.0f) : ov;
      const float A = as + ao, B = as * ts + ao * to, C = as * ts * ts + ao * to * to - 1.0f;
      const float det = B * B - A * C;
      if (det >= 0.0f) {
        const float u2 = (B + sqrtf(det)) / A;
        if (u2 > ov) r = u2;
      }
    }
  }
  return base + (double)r;
}

// update_cell_local(axis_pick(ym1, ym2, yp1, yp2), axis_pick(xm1, xm2, xp1, xp2)) written for a short dependent instruction
// chain: the blocked round kernel below is bound by the latency of one evaluation (one wave advances the front one cell per
// iteration, and the waves of a tile share four SIMDs), and the form above compiles to ~245 instructions.  Same formulas;
// the picks through min / max / compare-select instead of nested updates, no structures passed by reference, the hardware's
// 1-ulp square root and a reciprocal constant (a + a' is 2, 3.25 or 4.5) instead of the correctly rounded sequences: the
// result differs from the form above by <= 2 ulp of a float around 1 (~2e-7 cell), below the 1e-6 cell at which stage B
// already treats a change as noise.  Values that must not feed the cell arrive as INFINITY (the caller reads them from a
// slot that holds it); SECOND = false: no second neighbours (stage A).
template <bool SECOND>
__device__ __forceinline__ double update_cell_local_fast(double ym1, double ym2, double yp1, double yp2, double xm1, double xm2,
                                                          double xp1, double xp2) {
  double v1y, v1x, v2y = INFINITY, v2x = INFINITY;
  if (SECOND) {
    // axis_pick: the j = -1 side unless the j = +1 side is strictly closer; the second neighbour of that side when it is not farther
    const bool ty = yp1 < ym1, tx = xp1 < xm1;
    v1y = ty ? yp1 : ym1;
    v1x = tx ? xp1 : xm1;
    const double c2y = ty ? yp2 : ym2, c2x = tx ? xp2 : xm2;
    v2y = (c2y <= v1y) ? c2y : INFINITY;
    v2x = (c2x <= v1x) ? c2x : INFINITY;
  } else {
    v1y = fmin(ym1, yp1);
    v1x = fmin(xm1, xp1);
  }
  // the axis with the smaller neighbour first (equal values: either)
  const double s1 = fmin(v1y, v1x), o1 = fmax(v1y, v1x);
  float as = 1.0f, ao = 1.0f, ts = 0.0f, r = 1.0f, rA = 0.5f;
  const float ov = (float)(o1 - s1);                                       // +inf when the other axis has no upwind neighbour
  float to = ov;
  if (SECOND) {
    const bool y_first = v1y <= v1x;
    const double s2v = y_first ? v2y : v2x, o2v = y_first ? v2x : v2y;
    const bool s2 = s2v < INFINITY, o2 = o2v < INFINITY;
    as = s2 ? 2.25f : 1.0f;
    ts = s2 ? (float)(s1 - s2v) * (1.0f / 3.0f) : 0.0f;
    r = ts + (s2 ? (2.0f / 3.0f) : 1.0f);
    ao = o2 ? 2.25f : 1.0f;
    to = o2 ? ov + (float)(o1 - o2v) * (1.0f / 3.0f) : ov;
    rA = (s2 == o2) ? (s2 ? (1.0f / 4.5f) : 0.5f) : (1.0f / 3.25f);
  }
  const float A = as + ao, B = as * ts + ao * to, C = as * ts * ts + ao * to * to - 1.0f;
  // the two products pinned to registers of their own: hipcc otherwise forms (B, A) * (B, C) and takes the difference with a packed add
  // that reads the high register into its low half (op_sel) -- the form that is not safe beside fp16 / bf16 MFMA waves on gfx950
  // (common.h, PEANUT_NO_PK_F32; this kernel runs beside the prediction forward).  Same arithmetic: two products, one subtraction.
  float bb = B * B, ac = A * C;
  asm volatile("" : "+v"(bb), "+v"(ac));
  const float det = bb - ac;
  const float u2 = (B + __builtin_amdgcn_sqrtf(det)) * rA;
  if (ov < r && det >= 0.0f && u2 > ov) r = u2;                            // (ov = +inf: no joint root)
  return s1 < INFINITY ? s1 + (double)r : INFINITY;
}

// SECOND = false: stage A (first order, monotone).  SECOND = true: stage B (second order on the graph given by ord).
// Jacobi sweeps of the tile in LDS, one cell per lane.  A cell is only re-evaluated when one of the cells its stencil
// reads changed in the previous sweep (the update is a pure function of those and of its own value, so skipping it
// changes nothing): once the tile is loaded, the work follows the front -- a band a few cells wide -- instead of all
// 1024 cells, and with one 8 x 8 block per wave most waves skip a sweep altogether.  Only a ring of tiles is awake in
// a round (<= 64 of 900 on the agent's map), so a round costs the LATENCY of one tile: sweeps x time per sweep; hence
// one evaluation per lane (1024 lanes) rather than four, the feed predicates hoisted out of the sweeps, and the
// quadratic solved in single precision relative to the smaller upwind value (update_cell_local).  `active_clear`
// (the flags of the round after next) is wiped here, one byte per tile, which saves a fill launch per round.
template <bool SECOND, bool LOCAL32>
__device__ __forceinline__ void fmm_round_body(double* __restrict__ dist, const double* __restrict__ ord,
                                               const unsigned char* __restrict__ state, int H, int W, int tiles_x, int tiles_y,
                                               const unsigned char* __restrict__ active_in, unsigned char* __restrict__ active_out,
                                               unsigned char* __restrict__ active_clear, unsigned int* __restrict__ changed_tiles) {
  const int tile = blockIdx.x;
  if (threadIdx.x == 0) active_clear[tile] = 0;
  if (!active_in[tile]) return;
  __shared__ double d[LT][LT + 1];
  __shared__ double o[SECOND ? LT : 1][LT + 1];
  __shared__ unsigned char st[LT][LT + 4];
  __shared__ unsigned char chg[2][LT][LT + 4];      // cells that changed in the previous / in this sweep (halo: never)
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int r0 = ty * TILE - HALO, c0 = tx * TILE - HALO;
  for (int i = threadIdx.x; i < LT * LT; i += 1024) {
    const int ly = i / LT, lx = i - ly * LT;
    const int r = r0 + ly, c = c0 + lx;
    const bool in = r >= 0 && r < H && c >= 0 && c < W;
    d[ly][lx] = in ? dist[(size_t)r * W + c] : INFINITY;
    if (SECOND) o[ly][lx] = in ? ord[(size_t)r * W + c] : INFINITY;
    st[ly][lx] = in ? state[(size_t)r * W + c] : ST_MASKED;
    chg[0][ly][lx] = 0;
    chg[1][ly][lx] = 0;
  }
  __syncthreads();
  // one cell per lane, one 8 x 8 block per wave (16 waves): a wave none of whose cells saw a change around it skips
  // the sweep as a whole, so the sweep costs one evaluation on the waves the front passes through and nothing elsewhere
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int ly = HALO + 8 * (wave >> 2) + (lane >> 3), lx = HALO + 8 * (wave & 3) + (lane & 7);
  // which neighbours may feed the cell: fixed for the round (state and `ord` do not change), so worked out once --
  // bit 0..3: y-1, y+1, x-1, x+1 precede the cell; bit 4..7: y-2, y+2, x-2, x+2 precede those; bit 8: the cell is
  // free.  Stage A: every neighbour may feed, second neighbours never.
  unsigned feed = st[ly][lx] == ST_FREE ? 0x100u : 0u;
  if (SECOND) {
    const double oi = o[ly][lx];
    const double oym = o[ly - 1][lx], oyp = o[ly + 1][lx], oxm = o[ly][lx - 1], oxp = o[ly][lx + 1];
    feed |= (oym < oi ? 1u : 0u) | (oyp < oi ? 2u : 0u) | (oxm < oi ? 4u : 0u) | (oxp < oi ? 8u : 0u);
    // (<=: two equal seeds in line feed the cell next to them; the graph stays acyclic, the first step is strict)
    feed |= (o[ly - 2][lx] <= oym ? 16u : 0u) | (o[ly + 2][lx] <= oyp ? 32u : 0u) | (o[ly][lx - 2] <= oxm ? 64u : 0u) |
            (o[ly][lx + 2] <= oxp ? 128u : 0u);
  } else {
    feed |= 0xfu;
  }
  bool ever = false;
  int sweeps = 0;
  for (; sweeps < MAX_SWEEPS; ++sweeps) {
    const int cur = sweeps & 1;
    const double old = d[ly][lx];
    double nv = old;
    bool need = sweeps == 0;        // a tile wakes because a neighbour changed its halo: everything once
    if (!need) {
      need = chg[cur][ly - 1][lx] | chg[cur][ly + 1][lx] | chg[cur][ly][lx - 1] | chg[cur][ly][lx + 1];
      if (SECOND) need |= chg[cur][ly - 2][lx] | chg[cur][ly + 2][lx] | chg[cur][ly][lx - 2] | chg[cur][ly][lx + 2];
    }
    if (need && (feed & 0x100u)) {
      // a neighbour feeds the cell only if it precedes it in `ord`; the second one only if it precedes the first
      const double ym1 = (feed & 1u) ? d[ly - 1][lx] : INFINITY, yp1 = (feed & 2u) ? d[ly + 1][lx] : INFINITY;
      const double xm1 = (feed & 4u) ? d[ly][lx - 1] : INFINITY, xp1 = (feed & 8u) ? d[ly][lx + 1] : INFINITY;
      double ym2 = INFINITY, yp2 = INFINITY, xm2 = INFINITY, xp2 = INFINITY;
      if (SECOND) {
        ym2 = (feed & 16u) ? d[ly - 2][lx] : INFINITY; yp2 = (feed & 32u) ? d[ly + 2][lx] : INFINITY;
        xm2 = (feed & 64u) ? d[ly][lx - 2] : INFINITY; xp2 = (feed & 128u) ? d[ly][lx + 2] : INFINITY;
      }
      double u;
      if (LOCAL32) u = update_cell_local(axis_pick(ym1, ym2, yp1, yp2), axis_pick(xm1, xm2, xp1, xp2));
      else u = update_cell(axis_term(ym1, ym2, yp1, yp2), axis_term(xm1, xm2, xp1, xp2));
      if (SECOND) {
        // changes at the rounding level of the update (1e-12 relative in double; 1e-6 cell with the single-precision
        // local solve) are noise, not information
        if (old < INFINITY && fabs(u - old) <= (LOCAL32 ? 1e-6 : 1e-12 * fmax(1.0, old))) u = old;
      } else {
        u = fmin(u, old);
      }
      nv = u;
    }
    const bool chd = nv != old;
    const int any = __syncthreads_or(chd);
    if (!any) break;
    ever = true;
    d[ly][lx] = nv;
    chg[cur ^ 1][ly][lx] = chd;
    __syncthreads();
  }
  if (!ever) return;      // (uniform: `ever` derives from __syncthreads_or)
  {
    const int r = r0 + ly, c = c0 + lx;
    if (r < H && c < W) dist[(size_t)r * W + c] = d[ly][lx];
  }
  if (threadIdx.x == 0) {
    atomicAdd(changed_tiles, 1u);
    if (sweeps == MAX_SWEEPS) active_out[tile] = 1;       // not settled inside the budget: go on next round
    if (ty > 0) active_out[tile - tiles_x] = 1;
    if (ty + 1 < tiles_y) active_out[tile + tiles_x] = 1;
    if (tx > 0) active_out[tile - 1] = 1;
    if (tx + 1 < tiles_x) active_out[tile + 1] = 1;
  }
}

template <bool SECOND, bool LOCAL32>
__global__ __launch_bounds__(1024) void fmm_round_kernel(double* __restrict__ dist, const double* __restrict__ ord,
                                                         const unsigned char* __restrict__ state, int H, int W, int tiles_x, int tiles_y,
                                                         const unsigned char* __restrict__ active_in, unsigned char* __restrict__ active_out,
                                                         unsigned char* __restrict__ active_clear, unsigned int* __restrict__ changed_tiles) {
  fmm_round_body<SECOND, LOCAL32>(dist, ord, state, H, W, tiles_x, tiles_y, active_in, active_out, active_clear, changed_tiles);
}
// The round of up to GB episodes: grid (tiles, E).  `cur` = the rotation of the three flag arrays (the same for every episode: they
// take their rounds together); `counters` [E][MAX_ROUNDS_PER_CHECK], this round's column k.  An episode whose `done` bit is set
// returns at once, as a sleeping tile does.
template <bool SECOND, bool LOCAL32>
__global__ __launch_bounds__(1024) void fmm_round_batch_kernel(FieldBatchArgs a, int H, int W, int tiles_x, int tiles_y, int cur,
                                                               unsigned int* __restrict__ counters, int k) {
  const int e = blockIdx.y;
  if ((a.done >> e) & 1u) return;
  const int nt = tiles_x * tiles_y;
  unsigned char* act = a.active[e];
  fmm_round_body<SECOND, LOCAL32>(a.dist[e], a.ord[e], a.state[e], H, W, tiles_x, tiles_y, act + (size_t)cur * nt,
                                  act + (size_t)((cur + 1) % 3) * nt, act + (size_t)((cur + 2) % 3) * nt,
                                  counters + e * MAX_ROUNDS_PER_CHECK + k);
}

// The same round, blocked (round 5).  In the kernel above the front moves one cell per sweep and every sweep costs two
// workgroup barriers over 16 waves plus the change-tracking reads: ~1.1 us per sweep, 70-90 us for a front to cross a tile,
// and a round costs exactly that (only a ring of tiles is awake, so rounds are latency, not throughput).  Here a wave owns
// one 8 x 8 block of the tile and keeps a PRIVATE copy of it with its two-cell ring (12 x 12) in LDS: between two workgroup
// barriers it relaxes the block to convergence against the frozen ring -- Jacobi iterations inside the wave, which runs in
// lockstep, so they need no barrier at all (LDS operations of one wave execute in order) -- and then publishes the block.
// A front crosses a tile in 4-8 barrier pairs instead of 32-64, and an iteration costs the update alone.  A block is
// relaxed again only when one of its four neighbour blocks (the stencil is axis-aligned) published a change.  The
// schedule is deterministic (every block reads the tile as of the last barrier); stage A's monotone field and stage B's
// fixed dependency graph make the result independent of the schedule up to the update's own noise floor.
constexpr int BLK = 8, PT = BLK + 2 * HALO, MAX_OUTER = 64;      // private tile 12 x 12
template <bool SECOND, bool LOCAL32>
__device__ __forceinline__ void fmm_round_blocked_body(double* __restrict__ dist, const double* __restrict__ ord,
                                                       const unsigned char* __restrict__ state, int H, int W, int tiles_x, int tiles_y,
                                                       const unsigned char* __restrict__ active_in, unsigned char* __restrict__ active_out,
                                                       unsigned char* __restrict__ active_clear, unsigned int* __restrict__ changed_tiles,
                                                       int max_inner) {
  const int tile = blockIdx.x;
  if (threadIdx.x == 0) active_clear[tile] = 0;
  if (!active_in[tile]) return;
  __shared__ double d[LT][LT + 1];
  __shared__ double o[SECOND ? LT : 1][LT + 1];
  __shared__ unsigned char st[LT][LT + 4];
  __shared__ double priv[16][PT * (PT + 1) + 2];      // per wave: 12 rows of 13 (one of padding) + a slot that holds +inf
  __shared__ unsigned char blk[2][6][8];      // block (by, bx) at [by + 1][bx + 1]; the ring around the 4 x 4 blocks stays 0
  __shared__ int anyflag[2];
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int r0 = ty * TILE - HALO, c0 = tx * TILE - HALO;
  for (int i = threadIdx.x; i < LT * LT; i += 1024) {
    const int ly = i / LT, lx = i - ly * LT;
    const int r = r0 + ly, c = c0 + lx;
    const bool in = r >= 0 && r < H && c >= 0 && c < W;
    d[ly][lx] = in ? dist[(size_t)r * W + c] : INFINITY;
    if (SECOND) o[ly][lx] = in ? ord[(size_t)r * W + c] : INFINITY;
    st[ly][lx] = in ? state[(size_t)r * W + c] : ST_MASKED;
  }
  if (threadIdx.x < 2 * 6 * 8) (&blk[0][0][0])[threadIdx.x] = 0;
  if (threadIdx.x < 2) anyflag[threadIdx.x] = 0;
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // wave -> block through a Latin square (waves w, w + 4, w + 8, w + 12 share a SIMD): the blocks of a row AND of a column
  // of the tile sit on four different SIMDs, so a front that runs along either axis does not queue its blocks on one of them.
  // The square is SIMD = bx ^ m(by) with m = multiplication by x in GF(4) (0, 2, 3, 1: round 6), which also puts the two main
  // diagonals on four different SIMDs -- a front that crosses the tile obliquely; m = the Gray code (0, 1, 3, 2) of round 5 paired
  // them (solver on its own 1.92 / 1.84 -> 1.81 / 1.83 ms per call, beside the forward 4.52 / 4.54 -> 4.45 / 4.48: profiles/r9o).
  // Which wave relaxes a block does not enter the arithmetic.
  const int by = wave >> 2, bx = (wave & 3) ^ ((0x1320 >> (4 * by)) & 3);
  const int ly = HALO + BLK * by + (lane >> 3), lx = HALO + BLK * bx + (lane & 7);
  const int py = HALO + (lane >> 3), px = HALO + (lane & 7);
  unsigned feed = st[ly][lx] == ST_FREE ? 0x100u : 0u;       // as in fmm_round_kernel
  if (SECOND) {
    const double oi = o[ly][lx];
    const double oym = o[ly - 1][lx], oyp = o[ly + 1][lx], oxm = o[ly][lx - 1], oxp = o[ly][lx + 1];
    feed |= (oym < oi ? 1u : 0u) | (oyp < oi ? 2u : 0u) | (oxm < oi ? 4u : 0u) | (oxp < oi ? 8u : 0u);
    feed |= (o[ly - 2][lx] <= oym ? 16u : 0u) | (o[ly + 2][lx] <= oyp ? 32u : 0u) | (o[ly][lx - 2] <= oxm ? 64u : 0u) |
            (o[ly][lx + 2] <= oxp ? 128u : 0u);
  } else {
    feed |= 0xfu;
  }
  double* pv = priv[wave];
  constexpr int PS = PT + 1, INF_SLOT = PT * PS;
  if (lane == 0) pv[INF_SLOT] = INFINITY;
  // where the eight stencil values are read: the neighbour's cell of the private tile if it may feed this cell, the +inf slot if not
  const int pc = py * PS + px;
  const int a_ym1 = (feed & 1u) ? pc - PS : INF_SLOT, a_yp1 = (feed & 2u) ? pc + PS : INF_SLOT;
  const int a_xm1 = (feed & 4u) ? pc - 1 : INF_SLOT, a_xp1 = (feed & 8u) ? pc + 1 : INF_SLOT;
  const int a_ym2 = (feed & 16u) ? pc - 2 * PS : INF_SLOT, a_yp2 = (feed & 32u) ? pc + 2 * PS : INF_SLOT;
  const int a_xm2 = (feed & 64u) ? pc - 2 : INF_SLOT, a_xp2 = (feed & 128u) ? pc + 2 : INF_SLOT;
  const bool is_free = (feed & 0x100u) != 0;
  bool ever = false, again = false;      // again: the block's own iterations hit their cap
  int outer = 0;
  for (; outer < MAX_OUTER; ++outer) {
    const int cur = outer & 1, nxt = cur ^ 1;
    // the tile wakes because a neighbour changed its halo: every block once; afterwards only next to a published change
    const bool need = outer == 0 || again || blk[cur][by][bx + 1] || blk[cur][by + 2][bx + 1] || blk[cur][by + 1][bx] || blk[cur][by + 1][bx + 2];
    if (need) {      // (wave-uniform) private copy of the block and its ring, as of the last barrier
      for (int i = lane; i < PT * PT; i += 64) {
        const int qy = i / PT, qx = i - qy * PT;
        pv[qy * PS + qx] = d[BLK * by + qy][BLK * bx + qx];
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) anyflag[cur] = 0;
    if (lane == 0) blk[cur][by + 1][bx + 1] = 0;      // (read before the barrier above; written again in the next outer step)
    if (need) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      const double own0 = pv[pc];
      double val = own0;
      again = true;
      for (int inner = 0; inner < max_inner; ++inner) {
        const double ym1 = pv[a_ym1], yp1 = pv[a_yp1], xm1 = pv[a_xm1], xp1 = pv[a_xp1];
        double ym2 = INFINITY, yp2 = INFINITY, xm2 = INFINITY, xp2 = INFINITY;
        if (SECOND) { ym2 = pv[a_ym2]; yp2 = pv[a_yp2]; xm2 = pv[a_xm2]; xp2 = pv[a_xp2]; }
        double u;
        if (LOCAL32) u = update_cell_local_fast<SECOND>(ym1, ym2, yp1, yp2, xm1, xm2, xp1, xp2);
        else u = update_cell(axis_term(ym1, ym2, yp1, yp2), axis_term(xm1, xm2, xp1, xp2));
        if (SECOND) {
          if (val < INFINITY && fabs(u - val) <= (LOCAL32 ? 1e-6 : 1e-12 * fmax(1.0, val))) u = val;
        } else {
          u = fmin(u, val);
        }
        const double nv = is_free ? u : val;
        const bool chd = nv != val;
        if (!__any(chd)) { again = false; break; }
        // every lane has read before any lane writes (one instruction stream, LDS operations of a wave execute in order);
        // the next iteration reads after the write
        val = nv;
        asm volatile("" ::: "memory");
        pv[pc] = nv;
        asm volatile("" ::: "memory");
      }
      if (__any(val != own0)) {
        d[ly][lx] = val;
        if (lane == 0) { blk[nxt][by + 1][bx + 1] = 1; anyflag[nxt] = 1; }
      } else if (again && lane == 0) {
        anyflag[nxt] = 1;      // (cannot happen without a change; kept so that a capped block is never dropped)
      }
    }
    __syncthreads();
    if (!anyflag[nxt]) break;
    ever = true;
  }
  if (!ever) return;
  {
    const int r = r0 + ly, c = c0 + lx;
    if (r < H && c < W) dist[(size_t)r * W + c] = d[ly][lx];
  }
  if (threadIdx.x == 0) {
    atomicAdd(changed_tiles, 1u);
    if (outer == MAX_OUTER) active_out[tile] = 1;
    if (ty > 0) active_out[tile - tiles_x] = 1;
    if (ty + 1 < tiles_y) active_out[tile + tiles_x] = 1;
    if (tx > 0) active_out[tile - 1] = 1;
    if (tx + 1 < tiles_x) active_out[tile + 1] = 1;
  }
}

template <bool SECOND, bool LOCAL32>
__global__ __launch_bounds__(1024) void fmm_round_blocked_kernel(double* __restrict__ dist, const double* __restrict__ ord,
                                                                 const unsigned char* __restrict__ state, int H, int W, int tiles_x, int tiles_y,
                                                                 const unsigned char* __restrict__ active_in, unsigned char* __restrict__ active_out,
                                                                 unsigned char* __restrict__ active_clear, unsigned int* __restrict__ changed_tiles,
                                                                 int max_inner) {
  fmm_round_blocked_body<SECOND, LOCAL32>(dist, ord, state, H, W, tiles_x, tiles_y, active_in, active_out, active_clear, changed_tiles,
                                          max_inner);
}
template <bool SECOND, bool LOCAL32>
__global__ __launch_bounds__(1024) void fmm_round_blocked_batch_kernel(FieldBatchArgs a, int H, int W, int tiles_x, int tiles_y, int cur,
                                                                       unsigned int* __restrict__ counters, int k, int max_inner) {
  const int e = blockIdx.y;
  if ((a.done >> e) & 1u) return;
  const int nt = tiles_x * tiles_y;
  unsigned char* act = a.active[e];
  fmm_round_blocked_body<SECOND, LOCAL32>(a.dist[e], a.ord[e], a.state[e], H, W, tiles_x, tiles_y, act + (size_t)cur * nt,
                                          act + (size_t)((cur + 1) % 3) * nt, act + (size_t)((cur + 2) % 3) * nt,
                                          counters + e * MAX_ROUNDS_PER_CHECK + k, max_inner);
}

// stage B starts from the seeds again: distances back to +inf (seeds 0)
__device__ __forceinline__ void fmm_restart_body(const unsigned char* __restrict__ state, int n, double* __restrict__ dist) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) dist[i] = state[i] == ST_SEED ? 0.0 : INFINITY;
}
__global__ __launch_bounds__(256) void fmm_restart_kernel(const unsigned char* __restrict__ state, int n, double* __restrict__ dist) {
  fmm_restart_body(state, n, dist);
}
// What the host issues between two stages of the single solve (order <- dist; pass 0: the restart, the three flag arrays wiped, the
// seed tiles awake; later passes: every tile awake), for every episode that still takes passes, in one launch.  `cur`: the flag array
// the next round reads.
__global__ __launch_bounds__(256) void fmm_pass_batch_kernel(FieldBatchArgs a, int n, int nt, int restart, int cur) {
  const int e = blockIdx.y;
  if ((a.done >> e) & 1u) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) a.ord[e][i] = a.dist[e][i];
  if (restart) fmm_restart_body(a.state[e], n, a.dist[e]);
  if (i < nt) {
    unsigned char* act = a.active[e];
    const unsigned char wake = restart ? act[3 * (size_t)nt + i] : (unsigned char)1;
    for (int j = 0; j < 3; ++j) act[(size_t)j * nt + i] = j == cur ? wake : (unsigned char)0;
  }
}

// max over the reached cells (for `ma.filled(dd, np.max(dd) + 1)`); bits of a non-negative double order like an integer
__device__ __forceinline__ void fmm_max_body(const double* __restrict__ dist, int n, unsigned long long* __restrict__ max_bits) {
  double m = 0.0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const double v = dist[i];
    if (v < INFINITY && v > m) m = v;
  }
  for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) atomicMax(max_bits, (unsigned long long)__double_as_longlong(m));
}
__global__ __launch_bounds__(256) void fmm_max_kernel(const double* __restrict__ dist, int n, unsigned long long* __restrict__ max_bits) {
  fmm_max_body(dist, n, max_bits);
}
__global__ __launch_bounds__(256) void fmm_max_batch_kernel(FieldBatchArgs a, MaskBatchArgs m, int n) {
  const int e = blockIdx.y;
  if ((a.done >> e) & 1u) return;
  fmm_max_body(a.dist[e], n, m.max_bits[e]);
}
__device__ __forceinline__ void fmm_fill_body(const double* __restrict__ dist, int n, const unsigned long long* __restrict__ max_bits,
                                              double* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double v = dist[i];
  out[i] = v < INFINITY ? v : __longlong_as_double((long long)*max_bits) + 1.0;
}
__global__ __launch_bounds__(256) void fmm_fill_kernel(const double* __restrict__ dist, int n, const unsigned long long* __restrict__ max_bits,
                                                       double* __restrict__ out) {
  fmm_fill_body(dist, n, max_bits, out);
}
__global__ __launch_bounds__(256) void fmm_fill_batch_kernel(FieldBatchArgs a, MaskBatchArgs m, int n) {
  const int e = blockIdx.y;
  if ((a.done >> e) & 1u) return;
  fmm_fill_body(a.dist[e], n, m.max_bits[e], m.out[e]);
}

// max over ALL cells, +inf included (for `dd[dd == np.max(dd)] = np.inf` after the fill, :392-393): +inf when some cell is masked or
// unreached -- the rule then turns exactly those (filled with max + 1) into +inf, which they already are -- else the farthest
// reached distance, whose cells the rule turns into +inf too.  Bits of a non-negative double order like an integer.
__device__ __forceinline__ void goal_field_max_body(const double* __restrict__ dist, int n, unsigned long long* __restrict__ max_bits) {
  double m = 0.0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) m = fmax(m, dist[i]);
  for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
  if ((threadIdx.x & 63) == 0) atomicMax(max_bits, (unsigned long long)__double_as_longlong(m));
}
__global__ __launch_bounds__(256) void goal_field_max_kernel(const double* __restrict__ dist, int n, unsigned long long* __restrict__ max_bits) {
  goal_field_max_body(dist, n, max_bits);
}

// ---- weights over the local window: exp(-dd / temperature) (:395-396), their sum (:398) ----
// One partial sum per workgroup (fixed order inside it); goal_sum_kernel adds the partials in index order, so the sum -- and the
// "sum < 10: keep the last weights" decision -- is the same bits on every run.
__device__ __forceinline__ void goal_weight_body(const double* __restrict__ dist, int W, int gx1, int gy1, int lw, int lh,
                                                 double temperature, int frontier, const unsigned long long* __restrict__ field_max,
                                                 double* __restrict__ wt, double* __restrict__ part_out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const double dmax = __longlong_as_double((long long)*field_max);
  double w = 0.0;
  if (i < lw * lh) {
    const int r = i / lh, c = i - r * lh;
    double dd = dist[(size_t)(gx1 + r) * W + (gy1 + c)];
    if (dd == dmax) dd = INFINITY;      // (:393; a no-op unless every cell of the map was reached)
    if (frontier) {            // dist_weight_temperature == 0: frontier-based exploration (:404-406)
      if (dd < 60.0) dd = INFINITY;
      w = exp(-dd / 100.0);
    } else {
      w = exp(-dd / temperature);
    }
    wt[i] = w;
  }
  for (int o = 32; o > 0; o >>= 1) w += __shfl_xor(w, o);
  __shared__ double part[4];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) part_out[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}
__global__ __launch_bounds__(256) void goal_weight_kernel(const double* __restrict__ dist, int W, int gx1, int gy1, int lw, int lh,
                                                          double temperature, int frontier, const unsigned long long* __restrict__ field_max,
                                                          double* __restrict__ wt, double* __restrict__ part_out) {
  goal_weight_body(dist, W, gx1, gy1, lw, lh, temperature, frontier, field_max, wt, part_out);
}
// the partials of goal_weight_kernel in a fixed order: lane t adds t, t + 256, ... in turn, then a fixed tree
__device__ __forceinline__ void goal_sum_body(const double* __restrict__ part, int nparts, double* __restrict__ sum) {
  double w = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) w += part[i];
  for (int o = 32; o > 0; o >>= 1) w += __shfl_xor(w, o);
  __shared__ double p[4];
  if ((threadIdx.x & 63) == 0) p[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) *sum = (p[0] + p[1]) + (p[2] + p[3]);
}
__global__ __launch_bounds__(256) void goal_sum_kernel(const double* __restrict__ part, int nparts, double* __restrict__ sum) {
  goal_sum_body(part, nparts, sum);
}

// value = target_pred * dd_wt (or one of them alone) and its first-occurrence argmax (:401-413); two stages.
// np.argmax semantics: NaN ranks above every number (the first NaN wins), ties go to the smaller index.  The neutral element
// {-inf, INT_MAX} loses to every real candidate (-inf included, by index), so the result is always an index of the window.
struct ArgMax { double v; int i; };
__device__ __forceinline__ bool beats(ArgMax b, ArgMax a) {
  const bool bn = b.v != b.v, an = a.v != a.v;
  if (bn != an) return bn;
  return (bn || b.v == a.v) ? b.i < a.i : b.v > a.v;
}
__device__ __forceinline__ ArgMax better(ArgMax a, ArgMax b) { return beats(b, a) ? b : a; }
__device__ __forceinline__ void goal_argmax_body(const float* __restrict__ target_pred, const double* __restrict__ wt_new,
                                                 const double* __restrict__ wt_last, const double* __restrict__ sum, int have_last,
                                                 int mode, int n, double* __restrict__ value_out, ArgMax* __restrict__ partial) {
  // mode 0: target_pred * wt, 1: target_pred alone (temperature -1), 2: wt alone (temperature 0)
  const bool keep_last = mode != 2 && have_last && *sum < 10.0;      // (:398) "stuck inside obstacle, use last dd_wt"
  const double* wt = keep_last ? wt_last : wt_new;
  ArgMax best{-INFINITY, 0x7fffffff};
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const double tp = target_pred ? (double)target_pred[i] : 1.0;
    const double v = mode == 1 ? tp : (mode == 2 ? wt[i] : tp * wt[i]);
    if (value_out) value_out[i] = v;
    best = better(best, ArgMax{v, i});                // ascending i per lane: ties keep the first
  }
  for (int o = 32; o > 0; o >>= 1) {
    ArgMax other{__shfl_xor(best.v, o), __shfl_xor(best.i, o)};
    best = better(best, other);
  }
  __shared__ ArgMax part[4];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = better(better(part[0], part[1]), better(part[2], part[3]));
}
__global__ __launch_bounds__(256) void goal_argmax_kernel(const float* __restrict__ target_pred, const double* __restrict__ wt_new,
                                                          const double* __restrict__ wt_last, const double* __restrict__ sum, int have_last,
                                                          int mode, int n, double* __restrict__ value_out, ArgMax* __restrict__ partial) {
  goal_argmax_body(target_pred, wt_new, wt_last, sum, have_last, mode, n, value_out, partial);
}
__device__ __forceinline__ void goal_argmax_final_body(const ArgMax* __restrict__ partial, int nparts, const double* __restrict__ sum,
                                                       int have_last, int mode, const double* __restrict__ wt_new,
                                                       double* __restrict__ wt_last, int n, int* __restrict__ out_idx,
                                                       double* __restrict__ out_val) {
  ArgMax best{-INFINITY, 0x7fffffff};
  for (int i = threadIdx.x; i < nparts; i += 64) best = better(best, partial[i]);
  for (int o = 32; o > 0; o >>= 1) {
    ArgMax other{__shfl_xor(best.v, o), __shfl_xor(best.i, o)};
    best = better(best, other);
  }
  if (threadIdx.x == 0) {
    out_idx[0] = best.i;
    out_idx[1] = (mode != 2 && have_last && *sum < 10.0) ? 1 : 0;      // 1: the last weights were kept
    out_val[0] = best.v;
    out_val[1] = *sum;
  }
}
__global__ __launch_bounds__(64) void goal_argmax_final_kernel(const ArgMax* __restrict__ partial, int nparts, const double* __restrict__ sum,
                                                               int have_last, int mode, const double* __restrict__ wt_new,
                                                               double* __restrict__ wt_last, int n, int* __restrict__ out_idx,
                                                               double* __restrict__ out_val) {
  goal_argmax_final_body(partial, nparts, sum, have_last, mode, wt_new, wt_last, n, out_idx, out_val);
}

// ---- the same five for up to GB episodes: grid (what the single kernel takes, E) ----
struct GoalResult {             // per episode, read back in one copy
  unsigned long long field_max;
  double val[2];                // value max, sum of the fresh weights
  int idx[2];                   // argmax, 1 if the last weights were kept
};
struct SelectBatchArgs {
  const double* dist[GB];
  const float* target_pred[GB];
  double *wt_new[GB], *wt_last[GB], *wt_part[GB], *sum[GB], *value[GB];
  ArgMax* partial[GB];
  int gx1[GB], gy1[GB], have_last[GB];
  GoalResult* res;              // [E]
};
__global__ __launch_bounds__(256) void goal_field_max_batch_kernel(SelectBatchArgs a, int n) {
  const int e = blockIdx.y;
  goal_field_max_body(a.dist[e], n, &a.res[e].field_max);
}
__global__ __launch_bounds__(256) void goal_weight_batch_kernel(SelectBatchArgs a, int W, int lw, int lh, double temperature, int frontier) {
  const int e = blockIdx.y;
  goal_weight_body(a.dist[e], W, a.gx1[e], a.gy1[e], lw, lh, temperature, frontier, &a.res[e].field_max, a.wt_new[e], a.wt_part[e]);
}
__global__ __launch_bounds__(256) void goal_sum_batch_kernel(SelectBatchArgs a, int nparts) {
  const int e = blockIdx.y;
  goal_sum_body(a.wt_part[e], nparts, a.sum[e]);
}
__global__ __launch_bounds__(256) void goal_argmax_batch_kernel(SelectBatchArgs a, int mode, int n) {
  const int e = blockIdx.y;
  goal_argmax_body(a.target_pred[e], a.wt_new[e], a.wt_last[e], a.sum[e], a.have_last[e], mode, n, a.value[e], a.partial[e]);
}
__global__ __launch_bounds__(64) void goal_argmax_final_batch_kernel(SelectBatchArgs a, int nparts, int mode, int n) {
  const int e = blockIdx.y;
  goal_argmax_final_body(a.partial[e], nparts, a.sum[e], a.have_last[e], mode, a.wt_new[e], a.wt_last[e], n, a.res[e].idx, a.res[e].val);
}
// self.dd_wt = dd_wt (:410): the fresh weights become the last ones unless the old ones were kept -- the copy the single call
// issues after its read-back, decided on the device from the flag goal_argmax_final wrote
__global__ __launch_bounds__(256) void goal_keep_batch_kernel(SelectBatchArgs a, int n) {
  const int e = blockIdx.y;
  if (a.res[e].idx[1]) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) a.wt_last[e][i] = a.wt_new[e][i];
}

}  // namespace
}  // namespace peanut

using namespace peanut;

// What a batched select needs beyond the episodes' own handles; owned by the FIRST handle of the batch, made on first use.
struct GoalBatch {
  hipStream_t side = nullptr;              // as peanut_goal::side, for the fields of a begun batch
  hipEvent_t ev_inputs = nullptr, ev_field = nullptr;
  DevBuf counters, results;                // [GB][MAX_ROUNDS_PER_CHECK] "tiles changed" per episode and round; [GB] GoalResult
  unsigned int* host_counters = nullptr;   // pinned mirrors
  GoalResult* host_results = nullptr;
  // peanut_goal_select_begin_batch: what is on `side`, for whom and from which inputs
  struct Begun {
    bool on = false;
    int E = 0, batch = 0, cur = 0;
    peanut_goal* g[GB] = {nullptr};
    const float* obst[GB] = {nullptr};
    const unsigned char *col[GB] = {nullptr}, *vis[GB] = {nullptr};
    int lmb[GB][4] = {{0}}, loc[GB][2] = {{0}};
  } begun;
  ~GoalBatch() {
    if (ev_inputs) (void)hipEventDestroy(ev_inputs);
    if (ev_field) (void)hipEventDestroy(ev_field);
    if (side) (void)hipStreamDestroy(side);
    if (host_counters) (void)hipHostFree(host_counters);
    if (host_results) (void)hipHostFree(host_results);
  }
};
namespace { void drain_batch_of(peanut_goal* g); }

struct peanut_goal {
  peanut::Options opts = peanut::default_options();   // tuning options of this handle (options.h): snapshot at creation
  int H = 0, W = 0, rad = 0, tiles_x = 0, tiles_y = 0;
  DevBuf trav, state, dist, order, active, counters, maxbits, wt_new, wt_last, wt_part, sum, partial, out_idx, out_val, value;
  bool have_last = false;
  int last_lw = 0, last_lh = 0;
  int last_rounds = 0, last_passes = 0;
  bool last_converged = true;      // false: the ordering passes hit MAX_ORDER_PASSES with the last one still changing tiles
  int round_hint[1 + 64] = {0};    // rounds each stage needed in the previous solve (run_stage); stage 0 + up to 64 ordering passes (fmm_max_passes is clamped to 64)
  // peanut_goal_select_begin: the field of the next select is solved on `side`, behind `ev_inputs` only, so that it runs next to
  // whatever the caller enqueued on its stream after the call (the map-prediction forward that produces target_pred)
  hipStream_t side = nullptr;
  hipEvent_t ev_inputs = nullptr, ev_field = nullptr;
  unsigned int* host_counters = nullptr;   // pinned: the per-round counters of a batch land here without blocking the enqueuing thread
  // peanut_goal_select_begin: traversible map, initialisation and the first batch of stage-A rounds are already on `side`
  struct Begun {
    bool on = false;
    const float* obst = nullptr;
    const unsigned char *col = nullptr, *vis = nullptr;
    int lmb[4] = {0, 0, 0, 0}, loc_r = 0, loc_c = 0, batch = 0, cur = 0;
  } begun;
  std::shared_ptr<GoalBatch> batch;      // this handle leads batches (it is their first): their shared scratch
  std::shared_ptr<GoalBatch> begun_in;   // a begun batch this handle is part of: its rounds own the handle's scratch
  ~peanut_goal() {
    drain_batch_of(this);
    if (ev_inputs) (void)hipEventDestroy(ev_inputs);
    if (ev_field) (void)hipEventDestroy(ev_field);
    if (side) (void)hipStreamDestroy(side);
    if (host_counters) (void)hipHostFree(host_counters);
  }
};

namespace {

// A batch begun with this handle in it and not taken over: its rounds run out, and every handle of it is free again.
void drain_batch_of(peanut_goal* g) {
  if (!g->begun_in) return;
  std::shared_ptr<GoalBatch> B = g->begun_in;
  (void)hipStreamSynchronize(B->side);
  for (int e = 0; e < B->begun.E; ++e)
    if (B->begun.g[e]) { B->begun.g[e]->begun_in.reset(); B->begun.g[e] = nullptr; }
  B->begun.on = false;
  B->begun.E = 0;
}

// `batch` relaxation rounds of a stage and the read-back of their "tiles changed" counters, enqueued (no synchronisation)
template <bool SECOND>
int enqueue_rounds(peanut_goal* g, int* cur, int batch, hipStream_t s) {
  const int H = g->H, W = g->W, nt = g->tiles_x * g->tiles_y;
  unsigned char* act = (unsigned char*)g->active.p;
  unsigned int* counters = (unsigned int*)g->counters.p;
  if (!g->host_counters) PEANUT_HIP_CHECK(hipHostMalloc((void**)&g->host_counters, MAX_ROUNDS_PER_CHECK * sizeof(unsigned int), hipHostMallocDefault));
  PEANUT_HIP_CHECK(hipMemsetAsync(counters, 0, batch * sizeof(unsigned int), s));
  for (int k = 0; k < batch; ++k) {
    // three flag arrays in rotation: read, written (clean since the round before last), wiped for the next round
    unsigned char* in = act + (size_t)(*cur) * nt;
    unsigned char* out = act + (size_t)((*cur + 1) % 3) * nt;
    unsigned char* clr = act + (size_t)((*cur + 2) % 3) * nt;
    const bool local32 = opt(OPT_FMM_LOCAL32) != 0, blocked = opt(OPT_FMM_BLOCKED) != 0;
#define PEANUT_FMM_LAUNCH(KERNEL, ...)                                                                                                 \
  hipLaunchKernelGGL(KERNEL, dim3(nt), dim3(1024), 0, s, (double*)g->dist.p, (const double*)g->order.p, (const unsigned char*)g->state.p, \
                     H, W, g->tiles_x, g->tiles_y, in, out, clr, counters + k, ##__VA_ARGS__)
    if (blocked) {
      const int max_inner = (int)std::min<long long>(std::max<long long>(opt(OPT_FMM_INNER), 1), 1024);
      if (local32) PEANUT_FMM_LAUNCH((fmm_round_blocked_kernel<SECOND, true>), max_inner);
      else PEANUT_FMM_LAUNCH((fmm_round_blocked_kernel<SECOND, false>), max_inner);
    } else {
      if (local32) PEANUT_FMM_LAUNCH((fmm_round_kernel<SECOND, true>));
      else PEANUT_FMM_LAUNCH((fmm_round_kernel<SECOND, false>));
    }
#undef PEANUT_FMM_LAUNCH
    *cur = (*cur + 1) % 3;
  }
  PEANUT_HIP_CHECK(hipMemcpyAsync(g->host_counters, counters, batch * sizeof(unsigned int), hipMemcpyDeviceToHost, s));
  return 0;
}

// The host reads the per-round "tiles changed" counters once per batch of rounds.  The first batch of a stage is as long as that
// stage needed in the previous solve on this handle (+2: consecutive solves of an episode see almost the same map), so that a
// stage normally costs ONE host synchronisation; rounds after the field has settled wake no tile and cost a few microseconds each.
inline int first_batch(const peanut_goal* g, int stage) { return std::min(std::max(g->round_hint[stage] + 2, 4), MAX_ROUNDS_PER_CHECK); }

// rounds of one stage until a round changes nothing; *total = tiles changed over the whole stage.  enqueued > 0: the first batch
// (that many rounds) is already on the stream (peanut_goal_select_begin)
template <bool SECOND>
int run_stage(peanut_goal* g, int stage, int* cur, int* rounds_used, unsigned long long* total, hipStream_t s, int enqueued = 0) {
  const int max_rounds = 32 * (g->tiles_x + g->tiles_y) + 64;    // generous bound on the front's path, in tiles
  *total = 0;
  int batch = enqueued > 0 ? enqueued : first_batch(g, stage);
  int needed = 0;
  for (int round = 0; round < max_rounds; round += batch, batch = ROUNDS_PER_CHECK) {
    if (!(round == 0 && enqueued > 0))
      if (int rc = enqueue_rounds<SECOND>(g, cur, batch, s)) return rc;
    PEANUT_HIP_CHECK(hipStreamSynchronize(s));
    const unsigned int* host = g->host_counters;
    *rounds_used += batch;
    for (int k = 0; k < batch; ++k) {
      *total += host[k];
      if (host[k]) needed = round + k + 1;
    }
    if (host[batch - 1] == 0) {
      g->round_hint[stage] = needed;
      return 0;
    }
  }
  return fail(PEANUT_EHIP, "fmm: a relaxation stage did not settle within its round budget");
}

// state, distances and the seeds' tiles; leaves the seed tiles active in flag array 0
int field_preamble(peanut_goal* g, const unsigned char* trav, const unsigned char* seed_mask, int seed_r, int seed_c, hipStream_t s) {
  const int H = g->H, W = g->W, n = H * W, nt = g->tiles_x * g->tiles_y;
  unsigned char* act = (unsigned char*)g->active.p;     // three flag arrays in rotation (run_stage)
  unsigned char* seed_tiles = act + 3 * (size_t)nt;     // fourth array: the tiles that hold seeds
  PEANUT_HIP_CHECK(hipMemsetAsync(act, 0, 4 * (size_t)nt, s));
  hipLaunchKernelGGL(fmm_init_kernel, dim3((n + 255) / 256), dim3(256), 0, s, trav, seed_mask, seed_r, seed_c, H, W,
                     (unsigned char*)g->state.p, (double*)g->dist.p, seed_tiles, g->tiles_x);
  PEANUT_HIP_CHECK(hipMemcpyAsync(act, seed_tiles, nt, hipMemcpyDeviceToDevice, s));
  return 0;
}

// begun_batch > 0: the preamble and that many stage-A rounds are already on `s` (begun_cur = the flag rotation after them)
int solve_field(peanut_goal* g, const unsigned char* trav, const unsigned char* seed_mask, int seed_r, int seed_c, hipStream_t s,
                int begun_batch = 0, int begun_cur = 0) {
  const int H = g->H, W = g->W, n = H * W, nt = g->tiles_x * g->tiles_y;
  unsigned char* act = (unsigned char*)g->active.p;     // three flag arrays in rotation (run_stage)
  unsigned char* seed_tiles = act + 3 * (size_t)nt;     // fourth array: the tiles that hold seeds
  int cur = 0, rounds = 0;
  unsigned long long changed = 0;
  // stage A: first-order field
  if (begun_batch > 0) {
    cur = begun_cur;
  } else if (int rc = field_preamble(g, trav, seed_mask, seed_r, seed_c, s)) {
    return rc;
  }
  if (int rc = run_stage<false>(g, 0, &cur, &rounds, &changed, s, begun_batch)) return rc;
  // stage B: second order on the graph ordered by the previous field, until a pass changes nothing
  g->last_passes = 0;
  g->last_converged = false;
  const int max_passes = (int)std::min<long long>(std::max<long long>(opt(OPT_FMM_MAX_PASSES), 2), 64);
  for (int pass = 0; pass < max_passes; ++pass) {
    PEANUT_HIP_CHECK(hipMemcpyAsync(g->order.p, g->dist.p, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (pass == 0) {      // from the seeds again
      hipLaunchKernelGGL(fmm_restart_kernel, dim3((n + 255) / 256), dim3(256), 0, s, (const unsigned char*)g->state.p, n, (double*)g->dist.p);
      PEANUT_HIP_CHECK(hipMemsetAsync(act, 0, 3 * (size_t)nt, s));
      cur = 0;
      PEANUT_HIP_CHECK(hipMemcpyAsync(act, seed_tiles, nt, hipMemcpyDeviceToDevice, s));
    } else {              // warm start: every tile re-examines its cells under the new ordering
      PEANUT_HIP_CHECK(hipMemsetAsync(act + (size_t)cur * nt, 1, nt, s));
    }
    if (int rc = run_stage<true>(g, 1 + pass, &cur, &rounds, &changed, s)) return rc;
    g->last_passes = pass + 1;
    if (pass > 0 && changed == 0) { g->last_converged = true; break; }
  }
  g->last_rounds = rounds;
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(PEANUT_EHIP, std::string("fmm: ") + hipGetErrorString(e));
  return 0;
}

}  // namespace

extern "C" {

int peanut_goal_create(peanut_goal_t** out, int full_h, int full_w, int col_rad) {
  if (!out || full_h < 1 || full_w < 1 || col_rad < 0) return fail(PEANUT_EINVAL, "peanut_goal_create: bad arguments");
  auto g = std::make_unique<peanut_goal>();
  g->H = full_h; g->W = full_w; g->rad = col_rad;
  g->tiles_x = (full_w + TILE - 1) / TILE;
  g->tiles_y = (full_h + TILE - 1) / TILE;
  const size_t n = (size_t)full_h * full_w;
  int rc;
  if ((rc = g->trav.ensure(n)) || (rc = g->state.ensure(n)) || (rc = g->dist.ensure(n * sizeof(double))) ||
      (rc = g->order.ensure(n * sizeof(double))) || (rc = g->active.ensure(4 * (size_t)g->tiles_x * g->tiles_y)) || (rc = g->counters.ensure(MAX_ROUNDS_PER_CHECK * sizeof(unsigned int))) ||
      (rc = g->maxbits.ensure(2 * sizeof(unsigned long long))) || (rc = g->wt_new.ensure(n * sizeof(double))) ||
      (rc = g->wt_last.ensure(n * sizeof(double))) || (rc = g->wt_part.ensure((n + 255) / 256 * sizeof(double))) || (rc = g->value.ensure(n * sizeof(double))) || (rc = g->sum.ensure(sizeof(double))) ||
      (rc = g->partial.ensure(1024 * sizeof(ArgMax))) || (rc = g->out_idx.ensure(2 * sizeof(int))) || (rc = g->out_val.ensure(2 * sizeof(double))))
    return rc;
  *out = g.release();
  return 0;
}

void peanut_goal_destroy(peanut_goal_t* g) { delete g; }

int peanut_goal_reset(peanut_goal_t* g) {
  if (!g) return fail(PEANUT_EINVAL, "peanut_goal_reset: null handle");
  g->have_last = false;
  drain_batch_of(g);
  if (g->begun.on) { (void)hipStreamSynchronize(g->side); g->begun.on = false; }
  return 0;
}

namespace {
int ensure_side(peanut_goal* g) {
  if (g->side) return 0;
  // highest priority: the field is a chain of short launches (a ring of tiles per round) whose latency is the cost; its
  // workgroups should take the next free CU slots ahead of the forward's large grids
  int prio_least = 0, prio_greatest = 0;
  PEANUT_HIP_CHECK(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
  PEANUT_HIP_CHECK(hipStreamCreateWithPriority(&g->side, hipStreamNonBlocking, prio_greatest));
  PEANUT_HIP_CHECK(hipEventCreateWithFlags(&g->ev_inputs, hipEventDisableTiming));
  PEANUT_HIP_CHECK(hipEventCreateWithFlags(&g->ev_field, hipEventDisableTiming));
  return 0;
}
// np.clip(loc + lmb, 0, full - 1)  (:389-390)
void seed_cell(const peanut_goal* g, const int lmb[4], int loc_r, int loc_c, int* sr, int* sc) {
  int r = loc_r + lmb[0], c = loc_c + lmb[2];
  *sr = r < 0 ? 0 : (r > g->H - 1 ? g->H - 1 : r);
  *sc = c < 0 ? 0 : (c > g->W - 1 ? g->W - 1 : c);
}
}  // namespace

int peanut_goal_select_begin(peanut_goal_t* g, const float* full_obstacle, const uint8_t* collision_map, const uint8_t* visited_vis,
                             const int lmb[4], int loc_r, int loc_c, void* stream) {
  peanut::OptionScope option_scope(g ? &g->opts : nullptr);
  if (!g || !full_obstacle || !lmb) return fail(PEANUT_EINVAL, "peanut_goal_select_begin: null argument");
  if (lmb[0] < 0 || lmb[2] < 0 || lmb[1] > g->H || lmb[3] > g->W || lmb[1] - lmb[0] < 1 || lmb[3] - lmb[2] < 1)
    return fail(PEANUT_EINVAL, "peanut_goal_select_begin: bad local map boundaries");
  if (int rc = ensure_side(g)) return rc;
  drain_batch_of(g);
  if (g->begun.on) PEANUT_HIP_CHECK(hipStreamSynchronize(g->side));      // a begin nobody finished: its rounds still own the scratch
  PEANUT_HIP_CHECK(hipEventRecord(g->ev_inputs, (hipStream_t)stream));
  PEANUT_HIP_CHECK(hipStreamWaitEvent(g->side, g->ev_inputs, 0));
  // from here on work may be in flight on g->side that writes the handle's scratch: the handle is marked busy BEFORE the first
  // enqueue (for no inputs yet: obst = nullptr matches no select, so whoever comes next synchronises the side stream first), and an
  // enqueue that fails part-way lets the side stream run out before the error is returned
  g->begun.on = true;
  g->begun.obst = nullptr; g->begun.col = nullptr; g->begun.vis = nullptr;
  int cur = 0, batch = 0, rc = 0;
  int sr, sc;
  seed_cell(g, lmb, loc_r, loc_c, &sr, &sc);
  rc = peanut_goal_traversible(g, full_obstacle, collision_map, visited_vis, nullptr, g->side);
  if (!rc) rc = field_preamble(g, (const unsigned char*)g->trav.p, nullptr, sr, sc, g->side);
  if (!rc) { batch = first_batch(g, 0); rc = enqueue_rounds<false>(g, &cur, batch, g->side); }
  if (!rc && hipGetLastError() != hipSuccess) rc = fail(PEANUT_EHIP, "peanut_goal_select_begin: launch failed");
  if (rc) {
    (void)hipStreamSynchronize(g->side);
    g->begun.on = false;
    return rc;
  }
  g->begun.obst = full_obstacle; g->begun.col = collision_map; g->begun.vis = visited_vis;
  for (int i = 0; i < 4; ++i) g->begun.lmb[i] = lmb[i];
  g->begun.loc_r = loc_r; g->begun.loc_c = loc_c; g->begun.batch = batch; g->begun.cur = cur;
  return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------------------
// The solve of up to GB episodes in the launches and synchronisations of one (peanut_goal_select_batch).  Per episode the sequence
// of EFFECTIVE rounds is the one its own solve_field runs: a stage goes on until every episode's last counter of a check is zero --
// an episode that has settled takes no part in the stage's further rounds -- the next ordering pass starts for all episodes that
// still need one, and an episode whose pass changed nothing (pass > 0) is done.  Stage A is a monotone relaxation and stage B a
// fixed-point sweep on an acyclic graph: the field does not depend on when a round runs, so every episode ends with the bits of its
// own solve (tests/test_goal_batch_gpu.py holds that with torch.equal).
// ---------------------------------------------------------------------------------------------------------------------------------
namespace {

int ensure_batch(peanut_goal* lead) {
  if (lead->batch) return 0;
  auto B = std::make_shared<GoalBatch>();
  int prio_least = 0, prio_greatest = 0;      // (as ensure_side)
  PEANUT_HIP_CHECK(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
  PEANUT_HIP_CHECK(hipStreamCreateWithPriority(&B->side, hipStreamNonBlocking, prio_greatest));
  PEANUT_HIP_CHECK(hipEventCreateWithFlags(&B->ev_inputs, hipEventDisableTiming));
  PEANUT_HIP_CHECK(hipEventCreateWithFlags(&B->ev_field, hipEventDisableTiming));
  if (int rc = B->counters.ensure((size_t)GB * MAX_ROUNDS_PER_CHECK * sizeof(unsigned int))) return rc;
  if (int rc = B->results.ensure((size_t)GB * sizeof(GoalResult))) return rc;
  PEANUT_HIP_CHECK(hipHostMalloc((void**)&B->host_counters, (size_t)GB * MAX_ROUNDS_PER_CHECK * sizeof(unsigned int), hipHostMallocDefault));
  PEANUT_HIP_CHECK(hipHostMalloc((void**)&B->host_results, (size_t)GB * sizeof(GoalResult), hipHostMallocDefault));
  lead->batch = B;
  return 0;
}

// the refusals both batched entry points share; nothing is enqueued or waited for before they have passed
int check_batch(const char* who, int E, peanut_goal_t* const* g, const float* const* full_obstacle, const int* lmb, const int* loc_rc) {
  const std::string w(who);
  if (E < 1 || E > GB) return fail(PEANUT_EINVAL, w + ": E must be 1..PEANUT_GOAL_MAX_BATCH");
  if (!g || !full_obstacle || !lmb || !loc_rc) return fail(PEANUT_EINVAL, w + ": null argument");
  static const OptionId same[] = {OPT_FMM_BLOCKED, OPT_FMM_LOCAL32, OPT_FMM_INNER, OPT_FMM_MAX_PASSES};
  for (int e = 0; e < E; ++e) {
    if (!g[e] || !full_obstacle[e]) return fail(PEANUT_EINVAL, w + ": null handle or obstacle map");
    for (int f = 0; f < e; ++f)
      if (g[f] == g[e]) return fail(PEANUT_EINVAL, w + ": the same handle appears twice");
    if (g[e]->H != g[0]->H || g[e]->W != g[0]->W || g[e]->rad != g[0]->rad)
      return fail(PEANUT_EINVAL, w + ": the handles differ in map size or collision radius");
    for (OptionId id : same)
      if (g[e]->opts.v[id] != g[0]->opts.v[id]) return fail(PEANUT_EINVAL, w + ": the handles differ in their solver options");
    const int* b = lmb + 4 * e;
    if (b[0] < 0 || b[2] < 0 || b[1] > g[e]->H || b[3] > g[e]->W || b[1] - b[0] < 1 || b[3] - b[2] < 1)
      return fail(PEANUT_EINVAL, w + ": bad local map boundaries");
    if (b[1] - b[0] != lmb[1] - lmb[0] || b[3] - b[2] != lmb[3] - lmb[2])
      return fail(PEANUT_EINVAL, w + ": the local windows differ in size");
  }
  return 0;
}

// every begun piece of work (single or batch) on one of these handles runs out
void drain_all(int E, peanut_goal_t* const* g) {
  for (int e = 0; e < E; ++e) {
    drain_batch_of(g[e]);
    if (g[e]->begun.on) { (void)hipStreamSynchronize(g[e]->side); g[e]->begun.on = false; }
  }
}

void fill_field_args(int E, peanut_goal_t* const* g, const int* lmb, const int* loc_rc, FieldBatchArgs* fa, TravBatchArgs* ta,
                     const float* const* obst, const uint8_t* const* col, const uint8_t* const* vis) {
  *fa = FieldBatchArgs{};
  *ta = TravBatchArgs{};
  for (int e = 0; e < E; ++e) {
    fa->dist[e] = (double*)g[e]->dist.p; fa->ord[e] = (double*)g[e]->order.p;
    fa->state[e] = (unsigned char*)g[e]->state.p; fa->active[e] = (unsigned char*)g[e]->active.p;
    seed_cell(g[e], lmb + 4 * e, loc_rc[2 * e], loc_rc[2 * e + 1], &fa->seed_r[e], &fa->seed_c[e]);
    ta->obst[e] = obst[e]; ta->col[e] = col ? col[e] : nullptr; ta->vis[e] = vis ? vis[e] : nullptr;
    ta->trav[e] = (unsigned char*)g[e]->trav.p;
  }
}

// traversible maps + state, distances, seed tiles of all episodes: three launches
int field_preamble_batch(int E, peanut_goal* g0, const FieldBatchArgs& fa, const TravBatchArgs& ta, hipStream_t s) {
  const int H = g0->H, W = g0->W, n = H * W, nt = g0->tiles_x * g0->tiles_y;
  const dim3 tgrid((W + 31) / 32, (H + 7) / 8, E);
  if (g0->rad <= TRAV_MAX_RAD) hipLaunchKernelGGL(goal_trav_batch_kernel, tgrid, dim3(256), 0, s, ta, H, W, g0->rad);
  else hipLaunchKernelGGL(goal_trav_wide_batch_kernel, tgrid, dim3(256), 0, s, ta, H, W, g0->rad);
  hipLaunchKernelGGL(fmm_flags_clear_batch_kernel, dim3((4 * nt + 255) / 256, E), dim3(256), 0, s, fa, 4 * nt);
  hipLaunchKernelGGL(fmm_init_batch_kernel, dim3((n + 255) / 256, E), dim3(256), 0, s, fa, ta, H, W, g0->tiles_x, nt);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(PEANUT_EHIP, std::string("peanut_goal_select_batch: ") + hipGetErrorString(e));
}

// enqueue_rounds for the batch: one launch per round over (tiles, E), one read-back of the [E][MAX_ROUNDS_PER_CHECK] counters
template <bool SECOND>
int enqueue_rounds_batch(GoalBatch* B, int E, peanut_goal* g0, FieldBatchArgs fa, unsigned int skip, int* cur, int batch, hipStream_t s) {
  const int H = g0->H, W = g0->W, nt = g0->tiles_x * g0->tiles_y;
  unsigned int* counters = (unsigned int*)B->counters.p;
  const size_t bytes = (size_t)E * MAX_ROUNDS_PER_CHECK * sizeof(unsigned int);
  fa.done = skip;
  PEANUT_HIP_CHECK(hipMemsetAsync(counters, 0, bytes, s));
  const bool local32 = opt(OPT_FMM_LOCAL32) != 0, blocked = opt(OPT_FMM_BLOCKED) != 0;
  const int max_inner = (int)std::min<long long>(std::max<long long>(opt(OPT_FMM_INNER), 1), 1024);
  for (int k = 0; k < batch; ++k) {
#define PEANUT_FMM_LAUNCH(KERNEL, ...) \
  hipLaunchKernelGGL(KERNEL, dim3(nt, E), dim3(1024), 0, s, fa, H, W, g0->tiles_x, g0->tiles_y, *cur, counters, k, ##__VA_ARGS__)
    if (blocked) {
      if (local32) PEANUT_FMM_LAUNCH((fmm_round_blocked_batch_kernel<SECOND, true>), max_inner);
      else PEANUT_FMM_LAUNCH((fmm_round_blocked_batch_kernel<SECOND, false>), max_inner);
    } else {
      if (local32) PEANUT_FMM_LAUNCH((fmm_round_batch_kernel<SECOND, true>));
      else PEANUT_FMM_LAUNCH((fmm_round_batch_kernel<SECOND, false>));
    }
#undef PEANUT_FMM_LAUNCH
    *cur = (*cur + 1) % 3;
  }
  PEANUT_HIP_CHECK(hipMemcpyAsync(B->host_counters, counters, bytes, hipMemcpyDeviceToHost, s));
  return 0;
}

inline int first_batch_of(int E, peanut_goal_t* const* g, unsigned int skip, int stage) {
  int b = 4;
  for (int e = 0; e < E; ++e)
    if (!((skip >> e) & 1u)) b = std::max(b, first_batch(g[e], stage));
  return b;
}

// run_stage for the batch.  done: the episodes that take no part (bits >= E are set); changed[e] = tiles changed over the stage
template <bool SECOND>
int run_stage_batch(GoalBatch* B, int E, peanut_goal_t* const* g, const FieldBatchArgs& fa, int stage, unsigned int done, int* cur,
                    int* rounds_used, unsigned long long* changed, hipStream_t s, int enqueued = 0) {
  const int max_rounds = 32 * (g[0]->tiles_x + g[0]->tiles_y) + 64;
  int needed[GB] = {0};
  for (int e = 0; e < E; ++e) changed[e] = 0;
  unsigned int settled = done;
  int batch = enqueued > 0 ? enqueued : first_batch_of(E, g, done, stage);
  for (int round = 0; round < max_rounds; round += batch, batch = ROUNDS_PER_CHECK) {
    if (!(round == 0 && enqueued > 0))
      if (int rc = enqueue_rounds_batch<SECOND>(B, E, g[0], fa, settled, cur, batch, s)) return rc;
    PEANUT_HIP_CHECK(hipStreamSynchronize(s));
    *rounds_used += batch;
    for (int e = 0; e < E; ++e) {
      if ((settled >> e) & 1u) continue;
      const unsigned int* host = B->host_counters + (size_t)e * MAX_ROUNDS_PER_CHECK;
      for (int k = 0; k < batch; ++k) {
        changed[e] += host[k];
        if (host[k]) needed[e] = round + k + 1;
      }
      if (host[batch - 1] == 0) {
        g[e]->round_hint[stage] = needed[e];
        settled |= 1u << e;
      }
    }
    if (settled == 0xffffffffu) return 0;
  }
  return fail(PEANUT_EHIP, "fmm: a relaxation stage of the batch did not settle within its round budget");
}

// state, distances, seed tiles of the episodes not in fa.done, from given traversible maps and seed masks: two launches
int field_preamble_masks_batch(int E, peanut_goal* g0, const FieldBatchArgs& fa, const MaskBatchArgs& ma, hipStream_t s) {
  const int H = g0->H, W = g0->W, n = H * W, nt = g0->tiles_x * g0->tiles_y;
  hipLaunchKernelGGL(fmm_flags_clear_batch_kernel, dim3((4 * nt + 255) / 256, E), dim3(256), 0, s, fa, 4 * nt);
  hipLaunchKernelGGL(fmm_init_mask_batch_kernel, dim3((n + 255) / 256, E), dim3(256), 0, s, fa, ma, H, W, g0->tiles_x, nt);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(PEANUT_EHIP, std::string("fmm_distance_masks_batch: ") + hipGetErrorString(e));
}

// begun_batch > 0: the preamble and that many stage-A rounds are already on `s` (begun_cur = the flag rotation after them).
// skip: episodes (bits) that take no part at all -- their slots stay where they are, nothing of theirs is read or written but the
// flag arrays, which are scratch; masks: the preamble is the one on given masks (ta is not looked at)
int solve_field_batch(GoalBatch* B, int E, peanut_goal_t* const* g, const FieldBatchArgs& fa, const TravBatchArgs& ta, hipStream_t s,
                      int begun_batch, int begun_cur, unsigned int skip = 0u, const MaskBatchArgs* masks = nullptr) {
  const int n = g[0]->H * g[0]->W, nt = g[0]->tiles_x * g[0]->tiles_y;
  int cur = 0, rounds = 0;
  unsigned long long changed[GB];
  unsigned int done = (E >= 32 ? 0u : ~((1u << E) - 1u)) | skip;
  if (begun_batch > 0) {
    cur = begun_cur;
  } else if (masks) {
    FieldBatchArgs ia = fa;
    ia.done = done;
    if (int rc = field_preamble_masks_batch(E, g[0], ia, *masks, s)) return rc;
  } else if (int rc = field_preamble_batch(E, g[0], fa, ta, s)) {
    return rc;
  }
  if (int rc = run_stage_batch<false>(B, E, g, fa, 0, done, &cur, &rounds, changed, s, begun_batch)) return rc;
  for (int e = 0; e < E; ++e)
    if (!((skip >> e) & 1u)) { g[e]->last_passes = 0; g[e]->last_converged = false; }
  const int max_passes = (int)std::min<long long>(std::max<long long>(opt(OPT_FMM_MAX_PASSES), 2), 64);
  for (int pass = 0; pass < max_passes && done != 0xffffffffu; ++pass) {
    FieldBatchArgs pa = fa;
    pa.done = done;
    if (pass == 0) cur = 0;
    hipLaunchKernelGGL(fmm_pass_batch_kernel, dim3((n + 255) / 256, E), dim3(256), 0, s, pa, n, nt, pass == 0 ? 1 : 0, cur);
    if (int rc = run_stage_batch<true>(B, E, g, fa, 1 + pass, done, &cur, &rounds, changed, s)) return rc;
    for (int e = 0; e < E; ++e) {
      if ((done >> e) & 1u) continue;
      g[e]->last_passes = pass + 1;
      if (pass > 0 && changed[e] == 0) { g[e]->last_converged = true; done |= 1u << e; }
    }
  }
  for (int e = 0; e < E; ++e)
    if (!((skip >> e) & 1u)) g[e]->last_rounds = rounds;
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return fail(PEANUT_EHIP, std::string("fmm: ") + hipGetErrorString(err));
  return 0;
}

}  // namespace

// ---- the batched field on given masks (goal_internal.h): peanut_fmm_distance(g, trav, goal_mask, -1, -1, 1, out) for E handles ----
namespace peanut {

const char* fmm_masks_batch_bad(int E, peanut_goal_t* const* g) {
  if (E < 1 || E > GB) return "E must be 1..PEANUT_GOAL_MAX_BATCH";
  if (!g) return "null argument";
  static const OptionId same[] = {OPT_FMM_BLOCKED, OPT_FMM_LOCAL32, OPT_FMM_INNER, OPT_FMM_MAX_PASSES};
  for (int e = 0; e < E; ++e) {
    if (!g[e]) return "null solver handle";
    for (int f = 0; f < e; ++f)
      if (g[f] == g[e]) return "the same solver handle appears twice";
    if (g[e]->H != g[0]->H || g[e]->W != g[0]->W) return "the solver handles differ in map size";
    for (OptionId id : same)
      if (g[e]->opts.v[id] != g[0]->opts.v[id]) return "the solver handles differ in their solver options";
  }
  return nullptr;
}

int fmm_masks_batch_prepare(int E, peanut_goal_t* const* g) {
  if (const char* why = fmm_masks_batch_bad(E, g)) return fail(PEANUT_EINVAL, std::string("fmm_distance_masks_batch: ") + why);
  if (int rc = ensure_batch(g[0])) return rc;
  drain_all(E, g);
  return 0;
}

int fmm_distance_masks_batch(int E, peanut_goal_t* const* g, const unsigned char* const* trav, const unsigned char* const* seed_mask,
                             double* const* out, unsigned int skip, hipStream_t s) {
  if (const char* why = fmm_masks_batch_bad(E, g)) return fail(PEANUT_EINVAL, std::string("fmm_distance_masks_batch: ") + why);
  if (!trav || !seed_mask || !out) return fail(PEANUT_EINVAL, "fmm_distance_masks_batch: null argument");
  const unsigned int all = (1u << E) - 1u;
  skip &= all;
  if (skip == all) return 0;
  for (int e = 0; e < E; ++e)
    if (!((skip >> e) & 1u) && (!trav[e] || !seed_mask[e] || !out[e])) return fail(PEANUT_EINVAL, "fmm_distance_masks_batch: null map");
  peanut::OptionScope option_scope(&g[0]->opts);
  if (int rc = ensure_batch(g[0])) return rc;      // (made by fmm_masks_batch_prepare; a guard)
  GoalBatch* B = g[0]->batch.get();
  FieldBatchArgs fa{};
  TravBatchArgs ta{};
  MaskBatchArgs ma{};
  for (int e = 0; e < E; ++e) {
    fa.dist[e] = (double*)g[e]->dist.p; fa.ord[e] = (double*)g[e]->order.p;
    fa.state[e] = (unsigned char*)g[e]->state.p; fa.active[e] = (unsigned char*)g[e]->active.p;
    fa.seed_r[e] = -1; fa.seed_c[e] = -1;
    ma.trav[e] = trav[e]; ma.seed[e] = seed_mask[e]; ma.out[e] = out[e];
    ma.max_bits[e] = (unsigned long long*)g[e]->maxbits.p;
  }
  if (int rc = solve_field_batch(B, E, g, fa, ta, s, 0, 0, skip, &ma)) return rc;
  const int n = g[0]->H * g[0]->W;
  fa.done = ~all | skip;
  hipLaunchKernelGGL(fmm_max_batch_kernel, dim3(256, E), dim3(256), 0, s, fa, ma, n);
  hipLaunchKernelGGL(fmm_fill_batch_kernel, dim3((n + 255) / 256, E), dim3(256), 0, s, fa, ma, n);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(PEANUT_EHIP, std::string("fmm_distance_masks_batch: ") + hipGetErrorString(e));
}

}  // namespace peanut

extern "C" {

int peanut_goal_select_begin_batch(int E, peanut_goal_t* const* g, const float* const* full_obstacle, const uint8_t* const* collision_map,
                                   const uint8_t* const* visited_vis, const int* lmb, const int* loc_rc, void* stream) {
  if (int rc = check_batch("peanut_goal_select_begin_batch", E, g, full_obstacle, lmb, loc_rc)) return rc;
  peanut::OptionScope option_scope(&g[0]->opts);
  if (int rc = ensure_batch(g[0])) return rc;
  drain_all(E, g);
  GoalBatch* B = g[0]->batch.get();
  if (B->begun.on) (void)hipStreamSynchronize(B->side);      // (cannot be: a begun batch of this lead holds the lead; kept as a guard)
  PEANUT_HIP_CHECK(hipEventRecord(B->ev_inputs, (hipStream_t)stream));
  PEANUT_HIP_CHECK(hipStreamWaitEvent(B->side, B->ev_inputs, 0));
  // as peanut_goal_select_begin: the handles are marked busy BEFORE the first enqueue (with no inputs yet, which match no select),
  // and an enqueue that fails part-way lets the side stream run out before the error is returned
  GoalBatch::Begun& b = B->begun;
  b = GoalBatch::Begun{};
  b.on = true; b.E = E;
  for (int e = 0; e < E; ++e) { b.g[e] = g[e]; g[e]->begun_in = g[0]->batch; }
  FieldBatchArgs fa;
  TravBatchArgs ta;
  fill_field_args(E, g, lmb, loc_rc, &fa, &ta, full_obstacle, collision_map, visited_vis);
  int cur = 0, batch = 0;
  int rc = field_preamble_batch(E, g[0], fa, ta, B->side);
  if (!rc) { batch = first_batch_of(E, g, 0u, 0); rc = enqueue_rounds_batch<false>(B, E, g[0], fa, ~((E >= 32 ? 0u : (1u << E)) - 1u), &cur, batch, B->side); }
  if (!rc && hipGetLastError() != hipSuccess) rc = fail(PEANUT_EHIP, "peanut_goal_select_begin_batch: launch failed");
  if (rc) {
    drain_batch_of(g[0]);
    return rc;
  }
  for (int e = 0; e < E; ++e) {
    b.obst[e] = full_obstacle[e]; b.col[e] = collision_map ? collision_map[e] : nullptr; b.vis[e] = visited_vis ? visited_vis[e] : nullptr;
    for (int i = 0; i < 4; ++i) b.lmb[e][i] = lmb[4 * e + i];
    b.loc[e][0] = loc_rc[2 * e]; b.loc[e][1] = loc_rc[2 * e + 1];
  }
  b.batch = batch; b.cur = cur;
  return 0;
}

int peanut_goal_select_batch(int E, peanut_goal_t* const* g, const float* const* full_obstacle, const uint8_t* const* collision_map,
                             const uint8_t* const* visited_vis, const int* lmb, const int* loc_rc, const float* const* target_pred,
                             double dist_weight_temperature, int map_resolution, int* goal_rc_out, double* stats_out,
                             double* const* dist_out, double* const* value_out, void* stream) {
  if (int rc = check_batch("peanut_goal_select_batch", E, g, full_obstacle, lmb, loc_rc)) return rc;
  if (!goal_rc_out) return fail(PEANUT_EINVAL, "peanut_goal_select_batch: null argument");
  const int mode = dist_weight_temperature == -1 ? 1 : (dist_weight_temperature == 0 ? 2 : 0);
  if (mode != 2) {
    if (!target_pred) return fail(PEANUT_EINVAL, "peanut_goal_select_batch: target_pred is needed unless dist_weight_temperature == 0");
    for (int e = 0; e < E; ++e)
      if (!target_pred[e]) return fail(PEANUT_EINVAL, "peanut_goal_select_batch: target_pred is needed unless dist_weight_temperature == 0");
  }
  peanut::OptionScope option_scope(&g[0]->opts);
  if (int rc = ensure_batch(g[0])) return rc;
  hipStream_t s = (hipStream_t)stream;
  GoalBatch* B = g[0]->batch.get();
  // a batch begun for these very handles, in this order, with these very inputs is taken over; anything else runs out first
  bool aside = B->begun.on && B->begun.E == E && B->begun.batch > 0;
  for (int e = 0; aside && e < E; ++e) {
    const GoalBatch::Begun& b = B->begun;
    aside = b.g[e] == g[e] && g[e]->begun_in.get() == B && !g[e]->begun.on && b.obst[e] == full_obstacle[e] &&
            b.col[e] == (collision_map ? collision_map[e] : nullptr) && b.vis[e] == (visited_vis ? visited_vis[e] : nullptr) &&
            b.lmb[e][0] == lmb[4 * e] && b.lmb[e][1] == lmb[4 * e + 1] && b.lmb[e][2] == lmb[4 * e + 2] && b.lmb[e][3] == lmb[4 * e + 3] &&
            b.loc[e][0] == loc_rc[2 * e] && b.loc[e][1] == loc_rc[2 * e + 1];
  }
  FieldBatchArgs fa;
  TravBatchArgs ta;
  fill_field_args(E, g, lmb, loc_rc, &fa, &ta, full_obstacle, collision_map, visited_vis);
  if (aside) {
    const int begun_batch = B->begun.batch, begun_cur = B->begun.cur;
    for (int e = 0; e < E; ++e) { g[e]->begun_in.reset(); B->begun.g[e] = nullptr; }
    B->begun.on = false; B->begun.E = 0;
    if (int rc = solve_field_batch(B, E, g, fa, ta, B->side, begun_batch, begun_cur)) {
      (void)hipStreamSynchronize(B->side);      // `s` never joined the side stream: let it run out before the scratch is reused
      return rc;
    }
    PEANUT_HIP_CHECK(hipEventRecord(B->ev_field, B->side));
    PEANUT_HIP_CHECK(hipStreamWaitEvent(s, B->ev_field, 0));
  } else {
    drain_all(E, g);
    if (int rc = solve_field_batch(B, E, g, fa, ta, s, 0, 0)) return rc;
  }
  const int lw = lmb[1] - lmb[0], lh = lmb[3] - lmb[2], n = lw * lh;
  SelectBatchArgs sa{};
  sa.res = (GoalResult*)B->results.p;
  for (int e = 0; e < E; ++e) {
    peanut_goal* h = g[e];
    if (h->have_last && (h->last_lw != lw || h->last_lh != lh)) h->have_last = false;
    sa.dist[e] = (const double*)h->dist.p; sa.target_pred[e] = target_pred ? target_pred[e] : nullptr;
    sa.wt_new[e] = (double*)h->wt_new.p; sa.wt_last[e] = (double*)h->wt_last.p; sa.wt_part[e] = (double*)h->wt_part.p;
    sa.sum[e] = (double*)h->sum.p; sa.partial[e] = (ArgMax*)h->partial.p;
    sa.value[e] = value_out && value_out[e] ? value_out[e] : (double*)h->value.p;
    sa.gx1[e] = lmb[4 * e]; sa.gy1[e] = lmb[4 * e + 2]; sa.have_last[e] = h->have_last ? 1 : 0;
  }
  const double temperature = dist_weight_temperature / (double)map_resolution;      // (:395)
  const int nwt = (n + 255) / 256, nparts = std::min(1024, (n + 255) / 256);
  PEANUT_HIP_CHECK(hipMemsetAsync(B->results.p, 0, (size_t)E * sizeof(GoalResult), s));
  hipLaunchKernelGGL(goal_field_max_batch_kernel, dim3(256, E), dim3(256), 0, s, sa, g[0]->H * g[0]->W);
  hipLaunchKernelGGL(goal_weight_batch_kernel, dim3(nwt, E), dim3(256), 0, s, sa, g[0]->W, lw, lh, temperature, mode == 2 ? 1 : 0);
  hipLaunchKernelGGL(goal_sum_batch_kernel, dim3(1, E), dim3(256), 0, s, sa, nwt);
  hipLaunchKernelGGL(goal_argmax_batch_kernel, dim3(nparts, E), dim3(256), 0, s, sa, mode, n);
  hipLaunchKernelGGL(goal_argmax_final_batch_kernel, dim3(1, E), dim3(64), 0, s, sa, nparts, mode, n);
  if (mode != 2) hipLaunchKernelGGL(goal_keep_batch_kernel, dim3(nwt, E), dim3(256), 0, s, sa, n);
  PEANUT_HIP_CHECK(hipMemcpyAsync(B->host_results, B->results.p, (size_t)E * sizeof(GoalResult), hipMemcpyDeviceToHost, s));
  if (dist_out)
    for (int e = 0; e < E; ++e)
      if (dist_out[e]) PEANUT_HIP_CHECK(hipMemcpyAsync(dist_out[e], g[e]->dist.p, (size_t)g[e]->H * g[e]->W * sizeof(double), hipMemcpyDeviceToDevice, s));
  PEANUT_HIP_CHECK(hipStreamSynchronize(s));
  for (int e = 0; e < E; ++e) {
    const GoalResult& r = B->host_results[e];
    if (r.idx[0] < 0 || r.idx[0] >= n) return fail(PEANUT_EHIP, "peanut_goal_select_batch: argmax outside the local window");
    if (!r.idx[1] && mode != 2) { g[e]->last_lw = lw; g[e]->last_lh = lh; }
    if (mode != 2) g[e]->have_last = true;      // (frontier mode neither uses nor replaces the last weights)
    goal_rc_out[2 * e] = r.idx[0] / lh;
    goal_rc_out[2 * e + 1] = r.idx[0] - goal_rc_out[2 * e] * lh;
    if (stats_out) {
      stats_out[4 * e] = r.val[0]; stats_out[4 * e + 1] = r.val[1]; stats_out[4 * e + 2] = r.idx[1];
      stats_out[4 * e + 3] = g[e]->last_rounds;
    }
  }
  hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : fail(PEANUT_EHIP, std::string("peanut_goal_select_batch: ") + hipGetErrorString(err));
}

int peanut_goal_rounds(peanut_goal_t* g) { return g ? g->last_rounds : PEANUT_EINVAL; }
int peanut_goal_passes(peanut_goal_t* g) { return g ? g->last_passes : PEANUT_EINVAL; }
int peanut_goal_converged(peanut_goal_t* g) { return g ? (g->last_converged ? 1 : 0) : PEANUT_EINVAL; }

int peanut_fmm_distance(peanut_goal_t* g, const uint8_t* traversible, const uint8_t* goal_mask, int goal_r, int goal_c, int fill_mode,
                        double* dist_out, void* stream) {
  peanut::OptionScope option_scope(g ? &g->opts : nullptr);
  if (!g || !traversible || !dist_out) return fail(PEANUT_EINVAL, "peanut_fmm_distance: null argument");
  if (!goal_mask && (goal_r < 0 || goal_r >= g->H || goal_c < 0 || goal_c >= g->W))
    return fail(PEANUT_EINVAL, "peanut_fmm_distance: goal cell outside the map");
  hipStream_t s = (hipStream_t)stream;
  drain_batch_of(g);
  if (g->begun.on) { PEANUT_HIP_CHECK(hipStreamSynchronize(g->side)); g->begun.on = false; }      // (an unfinished select_begin owns the scratch)
  if (int rc = solve_field(g, traversible, goal_mask, goal_mask && goal_r < 0 ? -1 : goal_r, goal_c, s)) return rc;
  const int n = g->H * g->W;
  if (fill_mode == 0) {
    PEANUT_HIP_CHECK(hipMemcpyAsync(dist_out, g->dist.p, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s));
  } else {
    PEANUT_HIP_CHECK(hipMemsetAsync(g->maxbits.p, 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(fmm_max_kernel, dim3(256), dim3(256), 0, s, (const double*)g->dist.p, n, (unsigned long long*)g->maxbits.p);
    hipLaunchKernelGGL(fmm_fill_kernel, dim3((n + 255) / 256), dim3(256), 0, s, (const double*)g->dist.p, n,
                       (const unsigned long long*)g->maxbits.p, dist_out);
  }
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(PEANUT_EHIP, std::string("peanut_fmm_distance: ") + hipGetErrorString(e));
}

int peanut_goal_traversible(peanut_goal_t* g, const float* full_obstacle, const uint8_t* collision_map, const uint8_t* visited_vis,
                            uint8_t* trav_out, void* stream) {
  if (!g || !full_obstacle) return fail(PEANUT_EINVAL, "peanut_goal_traversible: null argument");
  if (g->rad <= TRAV_MAX_RAD)
    hipLaunchKernelGGL(goal_trav_kernel, dim3((g->W + 31) / 32, (g->H + 7) / 8), dim3(256), 0, (hipStream_t)stream, full_obstacle,
                       collision_map, visited_vis, g->H, g->W, g->rad, trav_out ? trav_out : (unsigned char*)g->trav.p);
  else
    hipLaunchKernelGGL(goal_trav_wide_kernel, dim3((g->W + 31) / 32, (g->H + 7) / 8), dim3(256), 0, (hipStream_t)stream, full_obstacle,
                       collision_map, visited_vis, g->H, g->W, g->rad, trav_out ? trav_out : (unsigned char*)g->trav.p);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(PEANUT_EHIP, std::string("peanut_goal_traversible: ") + hipGetErrorString(e));
}

int peanut_goal_select(peanut_goal_t* g, const float* full_obstacle, const uint8_t* collision_map, const uint8_t* visited_vis,
                       const int lmb[4], int loc_r, int loc_c, const float* target_pred, double dist_weight_temperature,
                       int map_resolution, int goal_rc_out[2], double stats_out[4], double* dist_out, double* value_out, void* stream) {
  peanut::OptionScope option_scope(g ? &g->opts : nullptr);
  if (!g || !full_obstacle || !lmb || !goal_rc_out) return fail(PEANUT_EINVAL, "peanut_goal_select: null argument");
  const int gx1 = lmb[0], gx2 = lmb[1], gy1 = lmb[2], gy2 = lmb[3];
  const int lw = gx2 - gx1, lh = gy2 - gy1;
  if (gx1 < 0 || gy1 < 0 || gx2 > g->H || gy2 > g->W || lw < 1 || lh < 1) return fail(PEANUT_EINVAL, "peanut_goal_select: bad local map boundaries");
  const int mode = dist_weight_temperature == -1 ? 1 : (dist_weight_temperature == 0 ? 2 : 0);
  if (mode != 2 && !target_pred) return fail(PEANUT_EINVAL, "peanut_goal_select: target_pred is needed unless dist_weight_temperature == 0");
  hipStream_t s = (hipStream_t)stream;
  int sr, sc;
  seed_cell(g, lmb, loc_r, loc_c, &sr, &sc);
  // the field needs the map inputs only: after peanut_goal_select_begin with these very inputs its traversible map, its
  // initialisation and the first batch of stage-A rounds are already running on the handle's own stream, next to what the caller
  // enqueued on `s` since (the forward that produces target_pred); the rest follows there and `s` joins before the weights
  bool aside = false;
  drain_batch_of(g);
  if (g->begun.on) {
    const peanut_goal::Begun& b = g->begun;
    aside = b.obst == full_obstacle && b.col == collision_map && b.vis == visited_vis && b.lmb[0] == gx1 && b.lmb[1] == gx2 &&
            b.lmb[2] == gy1 && b.lmb[3] == gy2 && b.loc_r == loc_r && b.loc_c == loc_c;
    g->begun.on = false;
    if (!aside) PEANUT_HIP_CHECK(hipStreamSynchronize(g->side));      // begun for other inputs: let it run out, solve these
  }
  if (aside) {
    if (int rc = solve_field(g, (const unsigned char*)g->trav.p, nullptr, sr, sc, g->side, g->begun.batch, g->begun.cur)) {
      (void)hipStreamSynchronize(g->side);      // `s` never joined the side stream: let it run out before the scratch is reused
      return rc;
    }
    PEANUT_HIP_CHECK(hipEventRecord(g->ev_field, g->side));
    PEANUT_HIP_CHECK(hipStreamWaitEvent(s, g->ev_field, 0));
  } else {
    if (int rc = peanut_goal_traversible(g, full_obstacle, collision_map, visited_vis, nullptr, stream)) return rc;
    if (int rc = solve_field(g, (const unsigned char*)g->trav.p, nullptr, sr, sc, s)) return rc;
  }
  if (g->have_last && (g->last_lw != lw || g->last_lh != lh)) g->have_last = false;
  const int n = lw * lh;
  const double temperature = dist_weight_temperature / (double)map_resolution;      // (:395)
  unsigned long long* field_max = (unsigned long long*)g->maxbits.p + 1;      // (slot 0: peanut_fmm_distance's fill)
  PEANUT_HIP_CHECK(hipMemsetAsync(field_max, 0, sizeof(unsigned long long), s));
  hipLaunchKernelGGL(goal_field_max_kernel, dim3(256), dim3(256), 0, s, (const double*)g->dist.p, g->H * g->W, field_max);
  const int nwt = (n + 255) / 256;
  hipLaunchKernelGGL(goal_weight_kernel, dim3(nwt), dim3(256), 0, s, (const double*)g->dist.p, g->W, gx1, gy1, lw, lh,
                     temperature, mode == 2 ? 1 : 0, (const unsigned long long*)field_max, (double*)g->wt_new.p, (double*)g->wt_part.p);
  hipLaunchKernelGGL(goal_sum_kernel, dim3(1), dim3(256), 0, s, (const double*)g->wt_part.p, nwt, (double*)g->sum.p);
  const int nparts = std::min(1024, (n + 255) / 256);
  hipLaunchKernelGGL(goal_argmax_kernel, dim3(nparts), dim3(256), 0, s, target_pred, (const double*)g->wt_new.p, (const double*)g->wt_last.p,
                     (const double*)g->sum.p, g->have_last ? 1 : 0, mode, n, value_out ? value_out : (double*)g->value.p, (ArgMax*)g->partial.p);
  hipLaunchKernelGGL(goal_argmax_final_kernel, dim3(1), dim3(64), 0, s, (const ArgMax*)g->partial.p, nparts, (const double*)g->sum.p,
                     g->have_last ? 1 : 0, mode, (const double*)g->wt_new.p, (double*)g->wt_last.p, n, (int*)g->out_idx.p, (double*)g->out_val.p);
  int idx[2];
  double val[2];
  PEANUT_HIP_CHECK(hipMemcpyAsync(idx, g->out_idx.p, sizeof(idx), hipMemcpyDeviceToHost, s));
  PEANUT_HIP_CHECK(hipMemcpyAsync(val, g->out_val.p, sizeof(val), hipMemcpyDeviceToHost, s));
  if (dist_out) PEANUT_HIP_CHECK(hipMemcpyAsync(dist_out, g->dist.p, (size_t)g->H * g->W * sizeof(double), hipMemcpyDeviceToDevice, s));
  PEANUT_HIP_CHECK(hipStreamSynchronize(s));
  if (idx[0] < 0 || idx[0] >= n) return fail(PEANUT_EHIP, "peanut_goal_select: argmax outside the local window");
  if (!idx[1] && mode != 2) {    // self.dd_wt = dd_wt (:410): the fresh weights become the last ones unless the old ones were kept
    PEANUT_HIP_CHECK(hipMemcpyAsync(g->wt_last.p, g->wt_new.p, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s));
    g->last_lw = lw; g->last_lh = lh;
  }
  if (mode != 2) g->have_last = true;      // (frontier mode neither uses nor replaces the last weights)
  goal_rc_out[0] = idx[0] / lh;
  goal_rc_out[1] = idx[0] - goal_rc_out[0] * lh;
  if (stats_out) { stats_out[0] = val[0]; stats_out[1] = val[1]; stats_out[2] = idx[1]; stats_out[3] = g->last_rounds; }
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(PEANUT_EHIP, std::string("peanut_goal_select: ") + hipGetErrorString(e));
}

// self.dd_wt / self.value (:409-410) where the last select left them: the visualisation frame (vis.hip) reads them in place
int peanut_goal_fields(peanut_goal_t* g, const double** dd_wt_out, const double** value_out, int dims_out[2]) {
  if (!g || !dd_wt_out || !value_out || !dims_out) return fail(PEANUT_EINVAL, "peanut_goal_fields: null argument");
  if (!g->have_last || !g->wt_last.p || !g->value.p)
    return fail(PEANUT_EINVAL, "peanut_goal_fields: no select has left weights on this handle (frontier mode keeps none)");
  *dd_wt_out = (const double*)g->wt_last.p;
  *value_out = (const double*)g->value.p;
  dims_out[0] = g->last_lw; dims_out[1] = g->last_lh;
  return 0;
}

}  // extern "C"
