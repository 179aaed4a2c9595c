// The local planner's short-term goal on the device: the reference's Agent_Helper._get_stg (nav/agent/agent_helper.py:374-493) and
// FMMPlanner.get_short_term_goal (nav/agent/utils/fmm_planner.py:77-116), which end every agent step.
//
// The reference does all of it on the host: a scikit-image dilation of the rounded obstacle map by the collision disk, the
// collision / visited overrides, a dilation of the goal map, a scikit-fmm solve on the (m + 2)^2 padded grid, an 11 x 11 window pick
// around the agent, and up to nine further solves when planning fails (the eroded retry, then the "make the goal larger" loop).
// Here three kernels stand around the solver of goal.hip, which is used through its own entry point (peanut_fmm_distance, goal mask,
// fill mode 1) and not forked:
//
//   * stg_trav_kernel: the planner's traversible map with the reference's border rules (the `grid[y1] = 1` quirk included), the
//     retry's erosion, the disk dilation as a ballot per row and an AND-test per chord (the scheme of goal.hip's goal_trav_body),
//     the overrides, the 3 x 3 start block with Python's slice semantics, and the ring of add_boundary;
//   * stg_goal_kernel: the goal mask, padded with zeros, dilated by a disk inside the padded grid;
//   * stg_window_kernel: get_short_term_goal on the device field, one workgroup, in double and in the reference's order; get_mask /
//     get_dist hold `d2 ** 0.5`, CPython's libm pow, so they are computed on the host (peanut_stg_masks) and travel in the
//     kernel-argument block.
//
// peanut_stg_plan is _get_stg's control flow over them; its loop conditions are host decisions on the 24-byte struct the window kernel
// wrote.  peanut_stg_plan_batch is the same for up to PEANUT_STG_MAX_BATCH episodes of a lock-step group, each with its own handle
// and its own state machine (StgEpisode), run in WAVES: the masks of every unfinished episode's next solve (the traversible maps of
// a wave in one launch, the grown goals in one), one batched solve on those masks (fmm_distance_masks_batch of goal.hip, declared in
// goal_internal.h), one window launch over the episodes, one read-back of the [E] window structs and one synchronisation; the
// host then advances every episode.  The waves of a call are the solves of its LONGEST chain, not of all chains in a row.  The
// window masks of 16 episodes (31 KB) do not fit the kernel-argument block: they go up once per call through a pinned table, and
// the window body reads them through a pointer in both forms.  All of it is binary morphology, comparisons and a handful of double operations without contraction: everything but the
// solver's field is held to the reference bit for bit.
#include <math.h>

#include <cmath>
#include <memory>
#include <string>

#include "goal_internal.h"
#include "net_common.h"

#pragma clang fp contract(off)

namespace peanut {
namespace {

constexpr int STG_MAX_RAD = PEANUT_STG_MAX_RAD;
constexpr int STG_MAX_SIDE = 2 * PEANUT_STG_MAX_STEP + 1;      // 11
constexpr int STG_MAX_CELLS = STG_MAX_SIDE * STG_MAX_SIDE;     // 121

// dilate(bit, disk(rad)) for the 8 x 32 cells of a workgroup of 256 threads; (r0, c0) = its first cell in the coordinates of `bit`,
// which answers false outside its grid.  The bits of the rows the block needs (8 + 2 rad of them, 32 + 2 rad <= 64 columns wide) are
// formed once with a ballot per row; a cell is hit when a row of its disk has a bit under that row's chord.  Every thread of the
// workgroup calls it (it holds the barrier); returns the answer for cell (r0 + tid / 32, c0 + tid % 32).
template <class Bit>
__device__ __forceinline__ bool disk_hit(Bit bit, int rad, int r0, int c0) {
  __shared__ unsigned long long rowbits[8 + 2 * STG_MAX_RAD];
  __shared__ int chord[2 * STG_MAX_RAD + 1];      // half-width of the disk at row offset dy
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int span = 32 + 2 * rad;
  for (int rr = wave; rr < 8 + 2 * rad; rr += 4) {
    const bool ob = lane < span && bit(r0 - rad + rr, c0 - rad + lane);
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
  bool hit = false;
  for (int dy = -rad; dy <= rad; ++dy) {
    const int w = chord[dy + rad];
    // bits lc + rad - w .. lc + rad + w of the row (bit b = column c0 - rad + b)
    const unsigned long long mask = ((w + w + 1 >= 64) ? ~0ull : ((1ull << (w + w + 1)) - 1ull)) << (lc + rad - w);
    hit = hit || (rowbits[lr + rad + dy] & mask) != 0ull;
  }
  return hit;
}

struct StgTravP {
  const float* obst;                          // [m, m], rs elements between rows
  const unsigned char *col, *vis;             // [full_w, full_h] or null
  unsigned char* out;                         // [(m + 2), (m + 2)]
  long long rs;
  int m, full_h, gx1, gy1;
  int row0, last_row, last_col;               // the border rules that apply (:382-390)
  int rad, erode;
  int blk_r0, blk_r1, blk_c0, blk_c1;         // the start block as half-open ranges (:417-418)
};

// Every kernel below exists twice, as in goal.hip: for one episode, and for up to SB episodes of a lock-step group in one launch
// (peanut_stg_plan_batch: the episode is a grid dimension, the per-episode arguments travel by value in SB slots).  Both are thin
// wrappers around ONE __device__ body.
constexpr int SB = PEANUT_STG_MAX_BATCH;

// grid (ceil((m + 2) / 32), ceil((m + 2) / 8)) over the PADDED output; the grid's cell is the padded one minus one
__device__ __forceinline__ void stg_trav_body(const StgTravP& p) {
  const int m = p.m, n = m + 2;
  // the bordered grid (:377-390): rint(obstacle) != 0, or a border rule
  auto grid_bit = [&](int r, int c) -> bool {
    if ((p.row0 && r == 0) || (p.last_row && r == m - 1) || (p.last_col && c == m - 1)) return true;
    return rintf(p.obst[(long long)r * p.rs + c]) != 0.f;
  };
  // ... eroded once for the retry (:448), cells outside the grid set; what the dilation sees, cells outside the grid unset
  auto bit = [&](int r, int c) -> bool {
    if ((unsigned)r >= (unsigned)m || (unsigned)c >= (unsigned)m) return false;
    if (!grid_bit(r, c)) return false;
    if (!p.erode) return true;
    return (r == 0 || grid_bit(r - 1, c)) && (r == m - 1 || grid_bit(r + 1, c)) && (c == 0 || grid_bit(r, c - 1)) &&
           (c == m - 1 || grid_bit(r, c + 1));
  };
  const int pr0 = blockIdx.y * 8, pc0 = blockIdx.x * 32;
  const bool blocked = disk_hit(bit, p.rad, pr0 - 1, pc0 - 1);
  const int pr = pr0 + (threadIdx.x >> 5), pc = pc0 + (threadIdx.x & 31);
  if (pr >= n || pc >= n) return;
  const int r = pr - 1, c = pc - 1;
  unsigned char t = 1;                        // the ring of add_boundary (:420)
  if ((unsigned)r < (unsigned)m && (unsigned)c < (unsigned)m) {
    t = blocked ? 0 : 1;
    const size_t at = (size_t)(p.gx1 + r) * p.full_h + (p.gy1 + c);
    if (p.col && p.col[at] == 1) t = 0;       // (:412-413)
    if (p.vis && p.vis[at] == 1) t = 1;       // (:414)
    if (r >= p.blk_r0 && r < p.blk_r1 && c >= p.blk_c0 && c < p.blk_c1) t = 1;
  }
  p.out[(size_t)pr * n + pc] = t;
}
__global__ __launch_bounds__(256) void stg_trav_kernel(const StgTravP p) { stg_trav_body(p); }
struct StgTravBatch { StgTravP p[SB]; };
// grid (.., .., slots): the maps one wave of the batch needs
__global__ __launch_bounds__(256) void stg_trav_batch_kernel(const StgTravBatch a) { stg_trav_body(a.p[blockIdx.z]); }

// grid as above; in: [m, m] (padded = 0) or [(m + 2), (m + 2)]
__device__ __forceinline__ void stg_goal_body(const unsigned char* __restrict__ in, int padded, int m, int rad,
                                              unsigned char* __restrict__ out) {
  const int n = m + 2;
  auto bit = [&](int pr, int pc) -> bool {
    if (padded) return (unsigned)pr < (unsigned)n && (unsigned)pc < (unsigned)n && in[(size_t)pr * n + pc] != 0;
    const int r = pr - 1, c = pc - 1;
    return (unsigned)r < (unsigned)m && (unsigned)c < (unsigned)m && in[(size_t)r * m + c] != 0;
  };
  const int pr0 = blockIdx.y * 8, pc0 = blockIdx.x * 32;
  const bool hit = disk_hit(bit, rad, pr0, pc0);
  const int pr = pr0 + (threadIdx.x >> 5), pc = pc0 + (threadIdx.x & 31);
  if (pr < n && pc < n) out[(size_t)pr * n + pc] = hit ? 1 : 0;
}
__global__ __launch_bounds__(256) void stg_goal_kernel(const unsigned char* __restrict__ in, int padded, int m, int rad,
                                                       unsigned char* __restrict__ out) {
  stg_goal_body(in, padded, m, rad, out);
}
struct StgGoalBatch {
  const unsigned char* in[SB];
  unsigned char* out[SB];
  int padded[SB], rad[SB];
};
__global__ __launch_bounds__(256) void stg_goal_batch_kernel(const StgGoalBatch a, int m) {
  const int j = blockIdx.z;
  stg_goal_body(a.in[j], a.padded[j], m, a.rad[j], a.out[j]);
}

struct StgMasks { double mask[STG_MAX_CELLS], dist[STG_MAX_CELLS]; };      // [(2 du + 1)^2] each, packed

// get_short_term_goal (fmm_planner.py:86-116): one workgroup of 128 threads, a thread per window cell.  The masks are read through
// a pointer: into the kernel-argument block in the single form, into the batch's device table in the other.
__device__ __forceinline__ void stg_window_body(const double* __restrict__ field, int n, int ir, int ic, int du, const StgMasks* Mp,
                                                peanut_stg_window_t* __restrict__ out) {
  const StgMasks& M = *Mp;
  __shared__ double sub[STG_MAX_CELLS];
  __shared__ double centre;
  const int side = 2 * du + 1, cells = side * side, t = threadIdx.x;
  const double n2 = (double)((long long)n * n);       // `fmm_dist.shape[0] ** 2`: np.pad's value and the masked-out value
  double v = 0.0;
  if (t < cells) {
    const int r = ir - du + t / side, c = ic - du + t % side;
    v = ((unsigned)r < (unsigned)n && (unsigned)c < (unsigned)n) ? field[(size_t)r * n + c] : n2;
    v = v * M.mask[t];                                // subset *= mask
    v = v + (1.0 - M.mask[t]) * n2;                   // subset += (1 - mask) * N ** 2
    if (t == du * side + du) centre = v;
  }
  __syncthreads();
  const double ce = centre;
  if (t < cells) {
    v = v - ce;                                       // subset -= subset[du, du]
    const double ratio = v / M.dist[t];
    if (ratio < -1.5) v = 1.0;                        // subset[ratio1 < -1.5] = 1
    sub[t] = v;
  }
  __syncthreads();
  if (t == 0) {                                       // np.argmin: first occurrence in row-major order, the first NaN wins
    int best = 0;
    double bv = sub[0];
    for (int i = 1; i < cells && bv == bv; ++i) {
      const double x = sub[i];
      if (x < bv || x != x) { bv = x; best = i; }
    }
    out->distance = ce;
    out->stg_r = best / side + ir - du;
    out->stg_c = best % side + ic - du;
    out->stop = ce < 5.0 ? 1 : 0;                     // 0.25 * 100 / 5.
    out->replan = bv > -0.0001 ? 1 : 0;
  }
}
__global__ __launch_bounds__(128) void stg_window_kernel(const double* __restrict__ field, int n, int ir, int ic, int du,
                                                         const StgMasks M, peanut_stg_window_t* __restrict__ out) {
  stg_window_body(field, n, ir, ic, du, &M, out);
}
struct StgWindowBatch {
  const double* field[SB];
  int ir[SB], ic[SB];
  unsigned int skip;              // bit e: episode e has no solve in this wave
};
// grid (E): masks [E] and out [E] are the batch's device tables, indexed by the episode
__global__ __launch_bounds__(128) void stg_window_batch_kernel(const StgWindowBatch a, int n, int du, const StgMasks* __restrict__ masks,
                                                               peanut_stg_window_t* __restrict__ out) {
  const int e = blockIdx.x;
  if ((a.skip >> e) & 1u) return;
  stg_window_body(a.field[e], n, a.ir[e], a.ic[e], du, masks + e, out + e);
}

// Python's a[i - 1:i + 2] on an axis of m cells, i >= 0, as a half-open range
void start_block(int i, int m, int* lo, int* hi) {
  int a = i - 1, b = i + 2;
  if (a < 0) a = a + m < 0 ? 0 : a + m;             // a negative start counts from the end: [-1:2] is empty for m >= 3
  *lo = a > m ? m : a;
  *hi = b > m ? m : b;
}

StgTravP trav_params(const float* obstacle, long long row_stride, int m, int full_w, int full_h, const int lmb[4], int col_rad, int erode,
                     const unsigned char* collision, const unsigned char* visited, int start_r, int start_c, unsigned char* trav_out) {
  StgTravP p{};
  p.obst = obstacle; p.col = collision; p.vis = visited; p.out = trav_out; p.rs = row_stride;
  p.m = m; p.full_h = full_h; p.gx1 = lmb[0]; p.gy1 = lmb[2];
  p.last_row = lmb[1] == full_w; p.last_col = lmb[3] == full_h;
  p.row0 = lmb[0] == 0 || lmb[2] == 0;              // `grid[x1] = 1` and `grid[y1] = 1` with x1 = y1 = 0: row 0 both times
  p.rad = col_rad; p.erode = erode ? 1 : 0;
  start_block(start_r, m, &p.blk_r0, &p.blk_r1);
  start_block(start_c, m, &p.blk_c0, &p.blk_c1);
  return p;
}

int trav_launch(const float* obstacle, long long row_stride, int m, int full_w, int full_h, const int lmb[4], int col_rad, int erode,
                const unsigned char* collision, const unsigned char* visited, int start_r, int start_c, unsigned char* trav_out,
                hipStream_t s) {
  const StgTravP p = trav_params(obstacle, row_stride, m, full_w, full_h, lmb, col_rad, erode, collision, visited, start_r, start_c, trav_out);
  const int n = m + 2;
  hipLaunchKernelGGL(stg_trav_kernel, dim3((n + 31) / 32, (n + 7) / 8), dim3(256), 0, s, p);
  return 0;
}

const char* trav_args_bad(const float* obstacle, long long row_stride, int m, int full_w, int full_h, const int* lmb, int col_rad,
                          int start_r, int start_c) {
  if (!obstacle || !lmb) return "null argument";
  if (m < 3 || full_w < m || full_h < m) return "m must be >= 3 and fit the full map";
  if (row_stride < m) return "row_stride below m";
  if (lmb[0] < 0 || lmb[2] < 0 || lmb[1] > full_w || lmb[3] > full_h || lmb[1] - lmb[0] != m || lmb[3] - lmb[2] != m)
    return "lmb is not an m x m window inside the full map";
  if (col_rad < 0 || col_rad > STG_MAX_RAD) return "col_rad must be 0..PEANUT_STG_MAX_RAD";
  if (start_r < 0 || start_r >= m || start_c < 0 || start_c >= m) return "start outside [0, m)";
  return nullptr;
}

const char* window_args_bad(const double* field, int n, double state_r, double state_c, int step_size, const void* result) {
  if (!field || !result) return "null argument";
  if (n < 1 || n > 32768) return "n must be 1..32768";
  if (step_size < 1 || step_size > PEANUT_STG_MAX_STEP) return "step_size must be 1..PEANUT_STG_MAX_STEP";
  if (!(state_r >= 0.0 && state_r < (double)n && state_c >= 0.0 && state_c < (double)n)) return "int(state) outside [0, n)";
  return nullptr;
}

void stg_masks(double sx, double sy, int step_size, double* mask, double* dist) {
  const int size = 2 * step_size + 1, half = size / 2;
  const double hi = (double)(step_size * step_size), lo = (double)((step_size - 1) * (step_size - 1));
  for (int i = 0; i < size; ++i)
    for (int j = 0; j < size; ++j) {
      // ((i + 0.5) - (size // 2 + sx)) ** 2 + ((j + 0.5) - (size // 2 + sy)) ** 2
      const double d2 = std::pow(((double)i + 0.5) - ((double)half + sx), 2.0) + std::pow(((double)j + 0.5) - ((double)half + sy), 2.0);
      mask[i * size + j] = (d2 <= hi && d2 > lo) ? 1.0 : 0.0;
      double d = 1e-10;
      if (d2 <= hi) {
        const double root = std::pow(d2, 0.5);
        d = root > 5.0 ? root : 5.0;                // max(5, root); a NaN root keeps the 5 as Python's max does
      }
      dist[i * size + j] = d;
    }
  mask[half * size + half] = 1.0;
}

int window_launch(const double* field, int n, double state_r, double state_c, int step_size, peanut_stg_window_t* result_dev, hipStream_t s) {
  const int ir = (int)state_r, ic = (int)state_c;   // int(x): towards zero; the state is >= 0
  StgMasks M{};
  stg_masks(state_r - (double)ir, state_c - (double)ic, step_size, M.mask, M.dist);
  hipLaunchKernelGGL(stg_window_kernel, dim3(1), dim3(128), 0, s, field, n, ir, ic, step_size, M, result_dev);
  return 0;
}

int launched(const char* who) {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(PEANUT_EHIP, std::string(who) + ": " + hipGetErrorString(e));
}

}  // namespace
}  // namespace peanut

using namespace peanut;

// What a batched plan needs beyond the episodes' own handles; owned by the FIRST handle of the batch, made on first use.
struct StgBatch {
  DevBuf masks, results;                            // [SB] StgMasks, [SB] peanut_stg_window_t
  StgMasks* host_masks = nullptr;                   // pinned mirrors
  peanut_stg_window_t* host_results = nullptr;
  ~StgBatch() {
    if (host_masks) (void)hipHostFree(host_masks);
    if (host_results) (void)hipHostFree(host_results);
  }
};

struct peanut_stg {
  int m = 0, full_w = 0, full_h = 0, col_rad = 0, step_size = 0;
  int last_waves = 0;                               // synchronising waves of the last plan this handle took part in (peanut_stg_waves)
  std::unique_ptr<StgBatch> batch;                  // this handle leads batches (it is their first): their shared tables
  peanut_goal_t* solver = nullptr;                  // (m + 2) x (m + 2)
  DevBuf trav, goal[2], field, result;
  peanut_stg_window_t* host_result = nullptr;       // pinned
  ~peanut_stg() {
    if (solver) peanut_goal_destroy(solver);
    if (host_result) (void)hipHostFree(host_result);
  }
};

extern "C" {

int peanut_stg_traversible(const float* obstacle, long long row_stride, int m, int full_w, int full_h, const int lmb[4], int col_rad,
                           int erode, const uint8_t* collision, const uint8_t* visited, int start_r, int start_c, uint8_t* trav_out,
                           void* stream) {
  if (!trav_out) return fail(PEANUT_EINVAL, "peanut_stg_traversible: null argument");
  if (const char* why = trav_args_bad(obstacle, row_stride, m, full_w, full_h, lmb, col_rad, start_r, start_c))
    return fail(PEANUT_EINVAL, std::string("peanut_stg_traversible: ") + why);
  trav_launch(obstacle, row_stride, m, full_w, full_h, lmb, col_rad, erode, collision, visited, start_r, start_c, trav_out, (hipStream_t)stream);
  return launched("peanut_stg_traversible");
}

int peanut_stg_goal(const uint8_t* mask_in, int in_is_padded, int m, int radius, uint8_t* goal_out, void* stream) {
  if (!mask_in || !goal_out || mask_in == goal_out) return fail(PEANUT_EINVAL, "peanut_stg_goal: null argument, or goal_out is mask_in");
  if (m < 1 || radius < 0 || radius > STG_MAX_RAD || (in_is_padded != 0 && in_is_padded != 1))
    return fail(PEANUT_EINVAL, "peanut_stg_goal: m >= 1, radius 0..PEANUT_STG_MAX_RAD, in_is_padded 0 or 1");
  const int n = m + 2;
  hipLaunchKernelGGL(stg_goal_kernel, dim3((n + 31) / 32, (n + 7) / 8), dim3(256), 0, (hipStream_t)stream, mask_in, in_is_padded, m, radius,
                     goal_out);
  return launched("peanut_stg_goal");
}

int peanut_stg_masks(double sx, double sy, int step_size, double* mask_out, double* dist_out) {
  if (!mask_out || !dist_out) return fail(PEANUT_EINVAL, "peanut_stg_masks: null argument");
  if (step_size < 1 || step_size > PEANUT_STG_MAX_STEP) return fail(PEANUT_EINVAL, "peanut_stg_masks: step_size must be 1..PEANUT_STG_MAX_STEP");
  stg_masks(sx, sy, step_size, mask_out, dist_out);
  return 0;
}

int peanut_stg_window(const double* field, int n, double state_r, double state_c, int step_size, peanut_stg_window_t* result_dev,
                      void* stream) {
  if (const char* why = window_args_bad(field, n, state_r, state_c, step_size, result_dev))
    return fail(PEANUT_EINVAL, std::string("peanut_stg_window: ") + why);
  window_launch(field, n, state_r, state_c, step_size, result_dev, (hipStream_t)stream);
  return launched("peanut_stg_window");
}

int peanut_stg_create(peanut_stg_t** out, int m, int full_w, int full_h, int col_rad, int step_size) {
  if (!out || m < 1 || m > 32766 || full_w < m || full_h < m || col_rad < 0 || step_size < 1 || step_size > PEANUT_STG_MAX_STEP)
    return fail(PEANUT_EINVAL, "peanut_stg_create: bad arguments");
  auto h = std::make_unique<peanut_stg>();
  h->m = m; h->full_w = full_w; h->full_h = full_h; h->col_rad = col_rad; h->step_size = step_size;
  const size_t n2 = (size_t)(m + 2) * (m + 2);
  int rc;
  if ((rc = peanut_goal_create(&h->solver, m + 2, m + 2, 0)) || (rc = h->trav.ensure(n2)) || (rc = h->goal[0].ensure(n2)) ||
      (rc = h->goal[1].ensure(n2)) || (rc = h->field.ensure(n2 * sizeof(double))) || (rc = h->result.ensure(sizeof(peanut_stg_window_t))))
    return rc;
  PEANUT_HIP_CHECK(hipHostMalloc((void**)&h->host_result, sizeof(peanut_stg_window_t), hipHostMallocDefault));
  *out = h.release();
  return 0;
}

void peanut_stg_destroy(peanut_stg_t* h) { delete h; }

int peanut_stg_plan(peanut_stg_t* h, const float* obstacle, long long row_stride, const uint8_t* goal_map, const uint8_t* collision,
                    const uint8_t* visited, const int lmb[4], const double start_exact[2], int found_goal, int radius_found,
                    double magnify_when_hard, int max_magnify, peanut_stg_result_t* result_out, uint8_t* trav_out, uint8_t* goal_out,
                    double* dist_out, void* stream) {
  if (!h || !obstacle || !goal_map || !collision || !visited || !lmb || !start_exact || !result_out)
    return fail(PEANUT_EINVAL, "peanut_stg_plan: null argument");
  const int m = h->m, n = m + 2;
  if (m < 2 * h->step_size + 1) return fail(PEANUT_EINVAL, "peanut_stg_plan: m < 2 step_size + 1");
  if (!(start_exact[0] >= 0.0 && start_exact[0] < (double)m && start_exact[1] >= 0.0 && start_exact[1] < (double)m))
    return fail(PEANUT_EINVAL, "peanut_stg_plan: start_exact outside [0, m)");
  const int radius = found_goal == 1 ? radius_found : 2;      // (:425-430)
  if (radius < 0 || radius > STG_MAX_RAD) return fail(PEANUT_EINVAL, "peanut_stg_plan: goal radius must be 0..PEANUT_STG_MAX_RAD");
  const int sr = (int)start_exact[0], sc = (int)start_exact[1];
  if (const char* why = trav_args_bad(obstacle, row_stride, m, h->full_w, h->full_h, lmb, h->col_rad, sr, sc))
    return fail(PEANUT_EINVAL, std::string("peanut_stg_plan: ") + why);
  const double state_r = start_exact[0] + 1.0, state_c = start_exact[1] + 1.0;      // (:438)
  if (const char* why = window_args_bad((const double*)h->field.p, n, state_r, state_c, h->step_size, h->result.p))
    return fail(PEANUT_EINVAL, std::string("peanut_stg_plan: ") + why);
  hipStream_t s = (hipStream_t)stream;
  unsigned char* trav = (unsigned char*)h->trav.p;
  double* field = (double*)h->field.p;
  int cur = 0;                                      // which of goal[2] holds the current padded goal
  peanut_stg_window_t w{};
  int n_solves = 0;
  // planner.set_multi_goal(goal); planner.get_short_term_goal(state)
  auto solve = [&]() -> int {
    if (int rc = peanut_fmm_distance(h->solver, trav, (const uint8_t*)h->goal[cur].p, -1, -1, 1, field, s)) return rc;
    window_launch(field, n, state_r, state_c, h->step_size, (peanut_stg_window_t*)h->result.p, s);
    PEANUT_HIP_CHECK(hipMemcpyAsync(h->host_result, h->result.p, sizeof(w), hipMemcpyDeviceToHost, s));
    PEANUT_HIP_CHECK(hipStreamSynchronize(s));
    w = *h->host_result;
    ++n_solves;
    return 0;
  };
  trav_launch(obstacle, row_stride, m, h->full_w, h->full_h, lmb, h->col_rad, 0, collision, visited, sr, sc, trav, s);
  hipLaunchKernelGGL(stg_goal_kernel, dim3((n + 31) / 32, (n + 7) / 8), dim3(256), 0, s, goal_map, 0, m, radius, (unsigned char*)h->goal[cur].p);
  if (int rc = solve()) return rc;
  int retried = 0, n_magnify = 0;
  if (w.replan) {                                   // failed to plan a path: the eroded obstacle map (:443-469)
    retried = 1;
    trav_launch(obstacle, row_stride, m, h->full_w, h->full_h, lmb, h->col_rad, 1, collision, visited, sr, sc, trav, s);
    if (int rc = solve()) return rc;
  }
  if (found_goal == 1 && w.distance > magnify_when_hard) {      // make the goal larger (:473-489)
    int step = 0;
    while (w.distance > 100.0) {
      ++step;
      if (step > max_magnify) break;
      hipLaunchKernelGGL(stg_goal_kernel, dim3((n + 31) / 32, (n + 7) / 8), dim3(256), 0, s, (const unsigned char*)h->goal[cur].p, 1, m, 2,
                         (unsigned char*)h->goal[cur ^ 1].p);
      cur ^= 1;
      ++n_magnify;
      if (int rc = solve()) return rc;
    }
  }
  const size_t n2 = (size_t)n * n;
  if (trav_out) PEANUT_HIP_CHECK(hipMemcpyAsync(trav_out, trav, n2, hipMemcpyDeviceToDevice, s));
  if (goal_out) PEANUT_HIP_CHECK(hipMemcpyAsync(goal_out, h->goal[cur].p, n2, hipMemcpyDeviceToDevice, s));
  if (dist_out) PEANUT_HIP_CHECK(hipMemcpyAsync(dist_out, field, n2 * sizeof(double), hipMemcpyDeviceToDevice, s));
  if (trav_out || goal_out || dist_out) PEANUT_HIP_CHECK(hipStreamSynchronize(s));
  result_out->stg_x = (double)w.stg_r - 1.0;        // stg_x + x1 - 1 (:491)
  result_out->stg_y = (double)w.stg_c - 1.0;
  result_out->distance = w.distance;
  result_out->stop = w.stop;
  result_out->replan = w.replan;
  result_out->retried = retried;
  result_out->n_magnify = n_magnify;
  result_out->n_solves = n_solves;
  result_out->reserved = 0;
  h->last_waves = n_solves;
  return launched("peanut_stg_plan");
}

int peanut_stg_waves(peanut_stg_t* h) { return h ? h->last_waves : PEANUT_EINVAL; }

namespace {

int ensure_stg_batch(peanut_stg* lead) {
  if (lead->batch) return 0;
  auto B = std::make_unique<StgBatch>();
  if (int rc = B->masks.ensure((size_t)SB * sizeof(StgMasks))) return rc;
  if (int rc = B->results.ensure((size_t)SB * sizeof(peanut_stg_window_t))) return rc;
  PEANUT_HIP_CHECK(hipHostMalloc((void**)&B->host_masks, (size_t)SB * sizeof(StgMasks), hipHostMallocDefault));
  PEANUT_HIP_CHECK(hipHostMalloc((void**)&B->host_results, (size_t)SB * sizeof(peanut_stg_window_t), hipHostMallocDefault));
  lead->batch = std::move(B);
  return 0;
}

// one episode of the batch: _get_stg's control flow (peanut_stg_plan) as a state machine that is advanced once per wave
struct StgEpisode {
  enum Next { FIRST, RETRY, MAGNIFY, DONE } next = FIRST;      // the solve this episode takes in the coming wave
  int cur = 0, retried = 0, n_magnify = 0, n_solves = 0, step = 0, in_magnify = 0;
  peanut_stg_window_t w{};
  // after a solve whose window result is w: which solve follows (the conditions of peanut_stg_plan, in its order)
  void advance(int found_goal, double magnify_when_hard, int max_magnify) {
    ++n_solves;
    if (next == FIRST && w.replan) { next = RETRY; return; }               // failed to plan a path (:443-469)
    if (!in_magnify) {
      if (!(found_goal == 1 && w.distance > magnify_when_hard)) { next = DONE; return; }
      in_magnify = 1;                                                      // make the goal larger (:473-489)
    }
    if (!(w.distance > 100.0)) { next = DONE; return; }
    ++step;
    next = step > max_magnify ? DONE : MAGNIFY;
  }
};

}  // namespace

int peanut_stg_plan_batch(const peanut_stg_batch_t* b) {
  const char* who = "peanut_stg_plan_batch: ";
  if (!b || b->size != sizeof(peanut_stg_batch_t)) return fail(PEANUT_EINVAL, std::string(who) + "size is not sizeof(peanut_stg_batch_t)");
  const int E = b->E;
  if (E < 1 || E > SB) return fail(PEANUT_EINVAL, std::string(who) + "E must be 1..PEANUT_STG_MAX_BATCH");
  if (!b->h || !b->obstacle || !b->row_stride || !b->goal_map || !b->collision || !b->visited || !b->lmb || !b->start_exact ||
      !b->found_goal || !b->radius_found || !b->magnify_when_hard || !b->max_magnify || !b->result_out)
    return fail(PEANUT_EINVAL, std::string(who) + "null array");
  peanut_stg* const* h = b->h;
  peanut_goal_t* solver[SB];
  int radius[SB], sr[SB], sc[SB];
  double state_r[SB], state_c[SB];
  for (int e = 0; e < E; ++e) {
    if (!h[e] || !b->obstacle[e] || !b->goal_map[e] || !b->collision[e] || !b->visited[e]) return fail(PEANUT_EINVAL, std::string(who) + "null entry");
    for (int f = 0; f < e; ++f)
      if (h[f] == h[e]) return fail(PEANUT_EINVAL, std::string(who) + "the same handle appears twice");
    if (h[e]->m != h[0]->m || h[e]->full_w != h[0]->full_w || h[e]->full_h != h[0]->full_h || h[e]->col_rad != h[0]->col_rad ||
        h[e]->step_size != h[0]->step_size)
      return fail(PEANUT_EINVAL, std::string(who) + "the handles differ in m, full_w, full_h, col_rad or step_size");
    solver[e] = h[e]->solver;
  }
  const int m = h[0]->m, n = m + 2, step_size = h[0]->step_size;
  if (m < 2 * step_size + 1) return fail(PEANUT_EINVAL, std::string(who) + "m < 2 step_size + 1");
  for (int e = 0; e < E; ++e) {      // every per-episode condition peanut_stg_plan refuses
    const double* se = b->start_exact + 2 * e;
    if (!(se[0] >= 0.0 && se[0] < (double)m && se[1] >= 0.0 && se[1] < (double)m)) return fail(PEANUT_EINVAL, std::string(who) + "start_exact outside [0, m)");
    radius[e] = b->found_goal[e] == 1 ? b->radius_found[e] : 2;      // (:425-430)
    if (radius[e] < 0 || radius[e] > STG_MAX_RAD) return fail(PEANUT_EINVAL, std::string(who) + "goal radius must be 0..PEANUT_STG_MAX_RAD");
    sr[e] = (int)se[0]; sc[e] = (int)se[1];
    if (const char* why = trav_args_bad(b->obstacle[e], b->row_stride[e], m, h[e]->full_w, h[e]->full_h, b->lmb + 4 * e, h[e]->col_rad, sr[e], sc[e]))
      return fail(PEANUT_EINVAL, std::string(who) + why);
    state_r[e] = se[0] + 1.0; state_c[e] = se[1] + 1.0;              // (:438)
    if (const char* why = window_args_bad((const double*)h[e]->field.p, n, state_r[e], state_c[e], step_size, h[e]->result.p))
      return fail(PEANUT_EINVAL, std::string(who) + why);
  }
  if (const char* why = fmm_masks_batch_bad(E, solver)) return fail(PEANUT_EINVAL, std::string(who) + why);
  // nothing below refuses; what the call needs beyond the handles exists after these two (first use of this lead only)
  if (int rc = ensure_stg_batch(h[0])) return rc;
  if (int rc = fmm_masks_batch_prepare(E, solver)) return rc;
  hipStream_t s = (hipStream_t)b->stream;
  StgBatch* B = h[0]->batch.get();
  // a failure part-way: the stream runs out before the error returns (the tables and the handles' maps are free again)
  auto out = [&](int rc) -> int {
    if (rc) (void)hipStreamSynchronize(s);
    return rc;
  };
  // start_exact is fixed for the call: the window masks of all episodes go up once
  StgWindowBatch wa{};
  const unsigned char* trav[SB];
  const unsigned char* seed[SB];
  double* field[SB];
  for (int e = 0; e < E; ++e) {
    wa.ir[e] = (int)state_r[e]; wa.ic[e] = (int)state_c[e];          // int(x): towards zero; the state is >= 0
    wa.field[e] = (const double*)h[e]->field.p;
    stg_masks(state_r[e] - (double)wa.ir[e], state_c[e] - (double)wa.ic[e], step_size, B->host_masks[e].mask, B->host_masks[e].dist);
    trav[e] = (const unsigned char*)h[e]->trav.p;
    field[e] = (double*)h[e]->field.p;
  }
  if (hipMemcpyAsync(B->masks.p, B->host_masks, (size_t)E * sizeof(StgMasks), hipMemcpyHostToDevice, s) != hipSuccess)
    return out(fail(PEANUT_EHIP, std::string(who) + "the upload of the window masks failed"));
  StgEpisode ep[SB];
  const unsigned int all = (1u << E) - 1u;
  const dim3 mgrid2((n + 31) / 32, (n + 7) / 8);
  int waves = 0;
  for (;;) {
    // every unfinished episode prepares the masks of its next solve: the traversible maps of the wave in one launch, the goals in one
    StgTravBatch ta{};
    StgGoalBatch ga{};
    int nt = 0, ng = 0;
    unsigned int skip = 0u;
    for (int e = 0; e < E; ++e) {
      StgEpisode& x = ep[e];
      if (x.next == StgEpisode::DONE) { skip |= 1u << e; continue; }
      if (x.next == StgEpisode::FIRST || x.next == StgEpisode::RETRY) {
        if (x.next == StgEpisode::RETRY) x.retried = 1;
        ta.p[nt++] = trav_params(b->obstacle[e], b->row_stride[e], m, h[e]->full_w, h[e]->full_h, b->lmb + 4 * e, h[e]->col_rad,
                                 x.next == StgEpisode::RETRY ? 1 : 0, b->collision[e], b->visited[e], sr[e], sc[e], (unsigned char*)h[e]->trav.p);
      }
      if (x.next == StgEpisode::FIRST) {
        ga.in[ng] = b->goal_map[e]; ga.padded[ng] = 0; ga.rad[ng] = radius[e]; ga.out[ng] = (unsigned char*)h[e]->goal[x.cur].p;
        ++ng;
      } else if (x.next == StgEpisode::MAGNIFY) {
        ga.in[ng] = (const unsigned char*)h[e]->goal[x.cur].p; ga.padded[ng] = 1; ga.rad[ng] = 2; ga.out[ng] = (unsigned char*)h[e]->goal[x.cur ^ 1].p;
        ++ng;
        x.cur ^= 1;
        ++x.n_magnify;
      }
      seed[e] = (const unsigned char*)h[e]->goal[x.cur].p;
    }
    if (skip == all) break;
    if (nt) hipLaunchKernelGGL(stg_trav_batch_kernel, dim3(mgrid2.x, mgrid2.y, nt), dim3(256), 0, s, ta);
    if (ng) hipLaunchKernelGGL(stg_goal_batch_kernel, dim3(mgrid2.x, mgrid2.y, ng), dim3(256), 0, s, ga, m);
    // planner.set_multi_goal(goal); planner.get_short_term_goal(state), for the episodes of this wave
    if (int rc = fmm_distance_masks_batch(E, solver, trav, seed, field, skip, s)) return out(rc);
    wa.skip = skip;
    hipLaunchKernelGGL(stg_window_batch_kernel, dim3(E), dim3(128), 0, s, wa, n, step_size, (const StgMasks*)B->masks.p,
                       (peanut_stg_window_t*)B->results.p);
    if (hipMemcpyAsync(B->host_results, B->results.p, (size_t)E * sizeof(peanut_stg_window_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
      return out(fail(PEANUT_EHIP, std::string(who) + "the read-back of a wave failed"));
    ++waves;
    for (int e = 0; e < E; ++e) {
      if ((skip >> e) & 1u) continue;
      ep[e].w = B->host_results[e];
      ep[e].advance(b->found_goal[e], b->magnify_when_hard[e], b->max_magnify[e]);
    }
  }
  const size_t n2 = (size_t)n * n;
  bool taps = false;
  for (int e = 0; e < E; ++e) {
    uint8_t* t = b->trav_out ? b->trav_out[e] : nullptr;
    uint8_t* g = b->goal_out ? b->goal_out[e] : nullptr;
    double* d = b->dist_out ? b->dist_out[e] : nullptr;
    hipError_t err = hipSuccess;
    if (t) err = hipMemcpyAsync(t, h[e]->trav.p, n2, hipMemcpyDeviceToDevice, s);
    if (g && err == hipSuccess) err = hipMemcpyAsync(g, h[e]->goal[ep[e].cur].p, n2, hipMemcpyDeviceToDevice, s);
    if (d && err == hipSuccess) err = hipMemcpyAsync(d, h[e]->field.p, n2 * sizeof(double), hipMemcpyDeviceToDevice, s);
    if (err != hipSuccess) return out(fail(PEANUT_EHIP, std::string(who) + "a tap copy failed"));
    taps = taps || t || g || d;
  }
  if (taps) PEANUT_HIP_CHECK(hipStreamSynchronize(s));
  for (int e = 0; e < E; ++e) {
    const StgEpisode& x = ep[e];
    peanut_stg_result_t* r = b->result_out + e;
    r->stg_x = (double)x.w.stg_r - 1.0;        // stg_x + x1 - 1 (:491)
    r->stg_y = (double)x.w.stg_c - 1.0;
    r->distance = x.w.distance;
    r->stop = x.w.stop;
    r->replan = x.w.replan;
    r->retried = x.retried;
    r->n_magnify = x.n_magnify;
    r->n_solves = x.n_solves;
    r->reserved = 0;
    h[e]->last_waves = waves;
  }
  return launched("peanut_stg_plan_batch");
}

}  // extern "C"
