// The goal map of the planner inputs on the device: the reference's Agent_State.update_goal_map
// (nav/agent/agent_state.py:418-446), which decides on every step whether the agent has seen its object.
//
// The reference does it on the host: a device reduction (`local_map[cn].sum() != 0`), a copy of the goal category's plane to the
// host, `goal_erode` scikit-image erosions and one dilation there (4-connected cross; scikit-image calls
// scipy.ndimage.binary_erosion(border_value=1) / binary_dilation, so cells outside the map count as SET for the erosion and as
// UNSET for the dilation), a second device reduction over the category planes 4:10 for the "no other category claims the cell"
// mask, and `found_goal` from what is left.  All of it is binary morphology and one fp32 comparison, so this file holds it to the
// reference's own result bit for bit.
//
// Two launches for 1..PEANUT_MAP_MAX_BATCH episodes, no host synchronisation, no state:
//
//   * goal_map_morph_kernel, grid (tiles, E): a workgroup owns a 32 x 32 output tile of one episode.  It stages the tile plus a
//     halo of n_erode + 1 cells of `local_map[cn] > 0` into LDS as bytes (at most 50 x 50), runs every erosion and the dilation
//     there between two buffers -- the valid region shrinks by one ring per pass and ends as the tile -- and reads the other
//     category planes only for the tile's cells that the morphology left set.  A tile whose staged region holds no set cell is
//     written as zeros without a pass or a further read (most tiles of a real map).  The map is read through its plane and row
//     strides: after update_full_map the local map is a view into the full map.
//   * goal_map_finish_kernel, grid (E): one workgroup per episode ORs the goal map the first launch wrote (it is 230 KB at
//     480 x 480 and sits in L2), writes found[e], and where nothing was found marks the long-term goal cell.  The flag is taken
//     from the goal map itself rather than collected with atomics by the first launch: nothing has to be cleared beforehand (the
//     call assumes nothing about the previous contents of its outputs), and the kernel boundary is the only ordering needed.
//
// The reference's early-out (`local_map[cn].sum() != 0`) needs no launch of its own: the projection keeps the map non-negative,
// so a zero sum means no cell > 0, nothing survives, and found = 0 follows from the rule.
#include <string>

#include "../../include/peanut_hip.h"
#include "common.h"

namespace peanut {

namespace {

constexpr int GM_TILE = 32;
constexpr int GM_MAX_HALO = PEANUT_GOAL_MAP_MAX_ERODE + 1;
constexpr int GM_W = GM_TILE + 2 * GM_MAX_HALO;     // 50
constexpr int GM_PITCH = GM_W + 2;                  // 52
constexpr int GM_THREADS = 256;
constexpr int GM_FINISH_THREADS = 1024;

struct GoalMapP {
  const float* lm;        // [channels] planes of m x m, strided
  unsigned char* out;     // [m, m]
  long long ps, rs;       // plane / row stride in elements
  int cn, halo, n_erode, detect, gr, gc;      // halo = passes = morph ? n_erode + 1 : 0
};
struct GoalMapBatchArgs {
  GoalMapP p[PEANUT_MAP_MAX_BATCH];
};

__device__ __forceinline__ void goal_map_zero_tile(unsigned char* __restrict__ out, int m, int r0, int c0) {
  for (int idx = threadIdx.x; idx < GM_TILE * GM_TILE; idx += GM_THREADS) {
    const int r = r0 + idx / GM_TILE, c = c0 + idx % GM_TILE;
    if (r < m && c < m) out[(size_t)r * m + c] = 0;
  }
}

__global__ __launch_bounds__(GM_THREADS) void goal_map_morph_kernel(const GoalMapBatchArgs A, int channels, int m, int tiles_x) {
  __shared__ unsigned char buf[2][GM_W * GM_PITCH];
  const GoalMapP& p = A.p[blockIdx.y];
  const int r0 = (blockIdx.x / tiles_x) * GM_TILE, c0 = (blockIdx.x % tiles_x) * GM_TILE;
  if (!p.detect) {                  // only_explore: the finishing kernel marks the goal cell
    goal_map_zero_tile(p.out, m, r0, c0);
    return;
  }
  const int H = p.halo, W = GM_TILE + 2 * H;
  const float* __restrict__ own = p.lm + (long long)p.cn * p.ps;
  // S = local_map[cn] > 0 over the tile and its halo.  Outside the map: set while erosions follow, unset before the dilation
  const unsigned char outside0 = p.n_erode > 0 ? 1 : 0;
  int any = 0;
  for (int idx = threadIdx.x; idx < W * W; idx += GM_THREADS) {
    const int i = idx / W, j = idx - i * W;
    const int r = r0 - H + i, c = c0 - H + j;
    unsigned char v = outside0;
    if ((unsigned)r < (unsigned)m && (unsigned)c < (unsigned)m) {
      v = own[(long long)r * p.rs + c] > 0.f ? 1 : 0;
      any |= v;
    }
    buf[0][i * GM_PITCH + j] = v;
  }
  if (!__syncthreads_or(any)) {     // nothing set inside the map: erosion and dilation leave the tile empty
    goal_map_zero_tile(p.out, m, r0, c0);
    return;
  }
  int cur = 0;
  for (int k = 1; k <= H; ++k) {    // pass k is valid on [k, W - k)^2 and reads [k - 1, W - k + 1)^2 of pass k - 1
    const unsigned char* __restrict__ src = buf[cur];
    unsigned char* __restrict__ dst = buf[cur ^ 1];
    const int n = W - 2 * k;
    const bool erode = k <= p.n_erode;
    const unsigned char outside = k < p.n_erode ? 1 : 0;
    for (int idx = threadIdx.x; idx < n * n; idx += GM_THREADS) {
      const int i = k + idx / n, j = k + idx % n;
      const int r = r0 - H + i, c = c0 - H + j;
      const int o = i * GM_PITCH + j;
      const unsigned char ce = src[o], up = src[o - GM_PITCH], dn = src[o + GM_PITCH], le = src[o - 1], ri = src[o + 1];
      unsigned char v = outside;
      if ((unsigned)r < (unsigned)m && (unsigned)c < (unsigned)m) v = erode ? (ce & up & dn & le & ri) : (ce | up | dn | le | ri);
      dst[o] = v;
    }
    __syncthreads();
    cur ^= 1;
  }
  // S &= ((((((c4 + c5) + c6) + c7) + c8) + c9) - c[cn]) == 0, in fp32 in that order
  const unsigned char* __restrict__ src = buf[cur];
  const int c_end = channels < 10 ? channels : 10;
  for (int idx = threadIdx.x; idx < GM_TILE * GM_TILE; idx += GM_THREADS) {
    const int ti = idx / GM_TILE, tj = idx % GM_TILE;
    const int r = r0 + ti, c = c0 + tj;
    if (r >= m || c >= m) continue;
    unsigned char s = src[(H + ti) * GM_PITCH + H + tj];
    if (s) {
      const long long at = (long long)r * p.rs + c;
      float sum = p.lm[4 * p.ps + at];
      for (int ch = 5; ch < c_end; ++ch) sum = sum + p.lm[ch * p.ps + at];
      s = (sum - own[at]) == 0.f ? 1 : 0;
    }
    p.out[(size_t)r * m + c] = s;
  }
}

// found[e] = any(goal_map[e]); nothing found -> the long-term goal cell
__global__ __launch_bounds__(GM_FINISH_THREADS) void goal_map_finish_kernel(const GoalMapBatchArgs A, int m, int* __restrict__ found) {
  const GoalMapP& p = A.p[blockIdx.x];
  int any = 0;
  if (p.detect) {
    const size_t n = (size_t)m * m;
    if (((uintptr_t)p.out & 15) == 0) {
      const uint4* v = reinterpret_cast<const uint4*>(p.out);
      const size_t nv = n / 16;
      for (size_t i = threadIdx.x; i < nv; i += GM_FINISH_THREADS) {
        const uint4 q = v[i];
        any |= (q.x | q.y | q.z | q.w) != 0;
      }
      for (size_t i = nv * 16 + threadIdx.x; i < n; i += GM_FINISH_THREADS) any |= p.out[i];
    } else {
      for (size_t i = threadIdx.x; i < n; i += GM_FINISH_THREADS) any |= p.out[i];
    }
  }
  any = __syncthreads_or(any) ? 1 : 0;
  if (threadIdx.x == 0) {
    found[blockIdx.x] = any;
    if (!any) p.out[(size_t)p.gr * m + p.gc] = 1;
  }
}

// the argument checks for one episode (shared by the single and the batched call, which applies them to every episode before
// anything is enqueued)
int goal_map_params(GoalMapP& p, const float* local_map, int channels, int m, long long plane_stride, long long row_stride, int cn,
                    int morph, int n_erode, int detect, int goal_r, int goal_c, uint8_t* goal_map) {
  if (!local_map || !goal_map) return fail(PEANUT_EINVAL, "peanut_goal_map: null argument");
  if (channels < 5 || m < 1 || row_stride < m || plane_stride < (long long)(m - 1) * row_stride + m)
    return fail(PEANUT_EINVAL, "peanut_goal_map: bad dimensions or strides");
  if (cn < 4 || cn >= channels) return fail(PEANUT_EINVAL, "peanut_goal_map: cn must lie in [4, channels)");
  if ((morph != 0 && morph != 1) || (detect != 0 && detect != 1)) return fail(PEANUT_EINVAL, "peanut_goal_map: morph and detect are 0 or 1");
  if (n_erode < 0 || n_erode > PEANUT_GOAL_MAP_MAX_ERODE)
    return fail(PEANUT_EINVAL, "peanut_goal_map: n_erode must be 0..PEANUT_GOAL_MAP_MAX_ERODE");
  if (goal_r < 0 || goal_r >= m || goal_c < 0 || goal_c >= m) return fail(PEANUT_EINVAL, "peanut_goal_map: the goal cell is outside the map");
  p = GoalMapP{local_map, goal_map, plane_stride, row_stride, cn, morph ? n_erode + 1 : 0, morph ? n_erode : 0, detect, goal_r, goal_c};
  return 0;
}

int goal_map_launch(const GoalMapBatchArgs& A, int E, int channels, int m, int32_t* found, void* stream, const char* who) {
  const int tiles_x = (m + GM_TILE - 1) / GM_TILE;
  hipLaunchKernelGGL(goal_map_morph_kernel, dim3(tiles_x * tiles_x, E), dim3(GM_THREADS), 0, (hipStream_t)stream, A, channels, m, tiles_x);
  hipLaunchKernelGGL(goal_map_finish_kernel, dim3(E), dim3(GM_FINISH_THREADS), 0, (hipStream_t)stream, A, m, found);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(PEANUT_EHIP, std::string(who) + ": " + hipGetErrorString(e));
}

}  // namespace

}  // namespace peanut

using namespace peanut;

extern "C" int peanut_goal_map(const float* local_map, int channels, int m, long long plane_stride, long long row_stride, int cn, int morph,
                               int n_erode, int detect, int goal_r, int goal_c, uint8_t* goal_map, int32_t* found, void* stream) {
  if (!found) return fail(PEANUT_EINVAL, "peanut_goal_map: null argument");
  GoalMapBatchArgs A{};
  if (int rc = goal_map_params(A.p[0], local_map, channels, m, plane_stride, row_stride, cn, morph, n_erode, detect, goal_r, goal_c, goal_map))
    return rc;
  return goal_map_launch(A, 1, channels, m, found, stream, "peanut_goal_map");
}

extern "C" int peanut_goal_map_batch(int E, const float* const* local_maps, int channels, int m, const long long* plane_strides,
                                     const long long* row_strides, const int* params, uint8_t* const* goal_maps, int32_t* found,
                                     void* stream) {
  if (E < 1 || E > PEANUT_MAP_MAX_BATCH) return fail(PEANUT_EINVAL, "peanut_goal_map_batch: E must be 1..PEANUT_MAP_MAX_BATCH");
  if (!local_maps || !plane_strides || !row_strides || !params || !goal_maps || !found)
    return fail(PEANUT_EINVAL, "peanut_goal_map_batch: null argument");
  GoalMapBatchArgs A{};
  for (int e = 0; e < E; ++e) {
    const int* q = params + 6 * e;
    if (int rc = goal_map_params(A.p[e], local_maps[e], channels, m, plane_strides[e], row_strides[e], q[0], q[1], q[2], q[3], q[4], q[5],
                                 goal_maps[e]))
      return rc;
    for (int o = 0; o < e; ++o) {       // [goal_map, goal_map + m * m) of two episodes must not meet
      const uintptr_t a = (uintptr_t)goal_maps[o], b = (uintptr_t)goal_maps[e], n = (uintptr_t)m * m;
      if (a < b + n && b < a + n) return fail(PEANUT_EINVAL, "peanut_goal_map_batch: the goal maps of two episodes overlap");
    }
  }
  return goal_map_launch(A, E, channels, m, found, stream, "peanut_goal_map_batch");
}
