// The agent's visualisation frame (Agent_Helper._visualize, nav/agent/agent_helper.py:496-621) on the device.
//
// The reference builds it on the host: it downloads the semantic arg-max and three fields, runs a PIL palette pass, three
// matplotlib colour-map passes over m x m float64, three cv2.resize calls and a scikit-image dilation, and pastes the results into a
// 600 x 1415 BGR image.  Here the maps never leave the device and the frame is three small launches for 1..16 episodes (the episode
// is a grid dimension, the per-episode arguments travel by value as in plan.hip):
//
//   vis_index_kernel    one thread per cell of the window: the arg-max of the category planes and the rules of :518-543; the goal's
//                       disk(4) dilation from a 40 x 16 byte tile in LDS.  Reads planes 0, 1 and 4 .. 4 + ncat - 2 (the last category
//                       plane is a constant, planes 2 and 3 are not shown) + 3 byte planes, writes m x m bytes: 11 fp32 planes =
//                       10.1 MB + 0.7 MB in, 0.23 MB out at m = 480, ncat = 10.  Also resets the range words.
//   vis_range_kernel    NaN-propagating min / max of target_pred, value, dd_wt (np.min / np.max are exact, so any order gives their
//                       bits; -0 / +0 may differ in sign, which no later step can see: x - min and max - min are compared and
//                       divided only).  Wave reduction, then one 64-bit atomic min / max per wave on an order-preserving key.
//                       Reads 0.9 + 1.8 + 1.8 MB at m = 480 (fp32 prediction).
//   vis_compose_kernel  one thread per 8 consecutive bytes of the flat frame (2 547 000 = 8 * 318 375; rows are 4245 bytes, so a
//                       row-wise split would leave ragged stores): one 8-byte load of the background, the two to four pixels the
//                       bytes belong to overridden where a panel or the arrow covers them, one 8-byte store.  Reads the 2.5 MB
//                       background, 0.9 MB rgb, the index map and what the panels sample of the fields; writes 2.5 MB.
//
// Everything that decides a byte is integer arithmetic or one IEEE operation at a time: the normalisation is a subtraction and a
// division in the field's own type (contraction off), the scale by 256 is exact, the colour tables come from the host (the reference's
// k / 255 * 255 truncates one below k for several k, so nothing is recomputed here).  The arrow's vertices are formed by the caller
// in float64 (np.cos / np.sin own their last bit) and arrive as integers.
#include <algorithm>
#include <cmath>
#include <string>

#include "../../include/peanut_hip.h"
#include "common.h"

namespace peanut {

namespace {

constexpr int VH = PEANUT_VIS_H, VW = PEANUT_VIS_W;
constexpr int V_BYTES = PEANUT_VIS_FRAME_BYTES, V_CHUNKS = V_BYTES / 8;
static_assert(VH * VW * 3 == V_BYTES && V_BYTES % 8 == 0, "the frame is a whole number of 8-byte chunks");
constexpr int V_MAX_M = 4096;
constexpr int V_TX = 32, V_TY = 8, V_R = 4;                           // index kernel: tile and the radius of disk(4)
constexpr int V_LW = V_TX + 2 * V_R, V_LH = V_TY + 2 * V_R;           // 40 x 16 goal bytes in LDS
constexpr int V_RANGE_BLOCKS = 64;

struct VisEpP {
  const float* lm;
  long long ps, rs;
  const unsigned char* collision;            // at the window's first cell
  const unsigned char* visited;
  const unsigned char* goal;
  const unsigned char* rgb;
  const void* field[3];                      // target_pred, value, dd_wt
  unsigned char* index;
  unsigned long long* ranges;                // [0..5]: min / max keys of the three fields; [6]: bit f set = field f holds a NaN
  unsigned char* frame;
  int stg_r, stg_c;                          // resolved window cell, or -1: none
  int wide;                                  // bit f: field f is normalised in double
  int wdata;                                 // bit f: field f is stored as double
  int ax[4], ay[4];                          // arrow vertices
  int bx0, bx1, by0, by1;                    // their bounding box, clipped to the frame (empty: bx0 > bx1)
  unsigned arrow_bgr;
};
struct VisArgs {
  VisEpP p[PEANUT_VIS_MAX_BATCH];
  const unsigned char* background;
  const unsigned char* palette;
  const unsigned char* cmap;
  int m, ncat, full_h;
  double ifx_map, ifx_side;                  // 1.0 / (480.0 / m), 1.0 / (240.0 / m)
};
static_assert(sizeof(VisArgs) <= 3840, "the argument block must stay below 4 KiB with the hidden arguments");

// ---- 1. the index map ----
__device__ __forceinline__ int sem_argmax(const float* __restrict__ lm, long long ps, long long at, int ncat) {
  // vlm = local_map[4:]; vlm[-1] = 1e-5; vlm.argmax(0): the first maximum, NaN above every number
  float best = ncat > 1 ? lm[4 * ps + at] : 1e-5f;
  int arg = 0;
  for (int c = 1; c < ncat; ++c) {
    const float v = c == ncat - 1 ? 1e-5f : lm[(4 + c) * ps + at];
    if (v > best || (v != v && best == best)) { best = v; arg = c; }
  }
  return arg;
}

__global__ __launch_bounds__(V_TX * V_TY) void vis_index_kernel(const VisArgs A) {
  const VisEpP& p = A.p[blockIdx.z];
  const int m = A.m;
  __shared__ unsigned char g[V_LH][V_LW];
  const int tx = threadIdx.x, ty = threadIdx.y, t = ty * V_TX + tx;
  const int r0 = blockIdx.y * V_TY - V_R, c0 = blockIdx.x * V_TX - V_R;
  for (int k = t; k < V_LW * V_LH; k += V_TX * V_TY) {
    const int r = r0 + k / V_LW, c = c0 + k % V_LW;
    g[k / V_LW][k % V_LW] = ((unsigned)r < (unsigned)m && (unsigned)c < (unsigned)m) ? p.goal[(size_t)r * m + c] : 0;
  }
  if (blockIdx.x == 0 && blockIdx.y == 0 && t < PEANUT_VIS_RANGE_WORDS)      // the ranges start from the neutral keys
    p.ranges[t] = t < 6 ? ((t & 1) ? 0ull : ~0ull) : 0ull;
  __syncthreads();
  const int i = blockIdx.y * V_TY + ty, j = blockIdx.x * V_TX + tx;
  if (i >= m || j >= m) return;
  const long long at = (long long)i * p.rs + j;
  int sem = sem_argmax(p.lm, p.ps, at, A.ncat) + 5;                          // :518
  const size_t full = (size_t)i * A.full_h + j;
  if (p.collision[full] == 1) sem = 14;                                     // :519
  if (i == p.stg_r && j == p.stg_c) sem = 15;                               // :520-521
  if (sem == A.ncat + 4) {                                                  // :523-533
    sem = 0;
    if (rintf(p.lm[p.ps + at]) == 1.0f) sem = 2;
    if (rintf(p.lm[at]) == 1.0f) sem = 1;
  }
  if (p.visited[full] == 1) sem = 3;                                        // :535
  bool near_goal = false;                                                   // :538-543, disk(4): dr^2 + dc^2 <= 16
  for (int dr = -V_R; dr <= V_R; ++dr)
    for (int dc = -V_R; dc <= V_R; ++dc)
      if (dr * dr + dc * dc <= V_R * V_R && g[ty + V_R + dr][tx + V_R + dc]) near_goal = true;
  if (near_goal) sem = 4;
  p.index[(size_t)i * m + j] = (unsigned char)sem;
}

__global__ __launch_bounds__(256) void vis_sem_argmax_kernel(const float* __restrict__ lm, long long ps, long long rs, int ncat, int m,
                                                             unsigned char* __restrict__ out) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= m * m) return;
  const int i = k / m, j = k - i * m;
  out[k] = (unsigned char)sem_argmax(lm, ps, (long long)i * rs + j, ncat);
}

// ---- 2. the ranges ----
// an order-preserving map of the doubles (NaN excluded) onto unsigned integers, and back
__device__ __forceinline__ unsigned long long range_key(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double range_value(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

__global__ __launch_bounds__(256) void vis_range_kernel(const VisArgs A) {
  const VisEpP& p = A.p[blockIdx.z];
  const int f = blockIdx.y, n = A.m * A.m;
  const void* src = p.field[f];
  if (!src) return;
  const bool wide = (p.wdata >> f) & 1;
  unsigned long long lo = ~0ull, hi = 0ull;
  int nan = 0;
  for (int k = blockIdx.x * 256 + threadIdx.x; k < n; k += gridDim.x * 256) {
    const double v = wide ? ((const double*)src)[k] : (double)((const float*)src)[k];       // float -> double is exact
    if (v != v) { nan = 1; continue; }
    const unsigned long long key = range_key(v);
    lo = key < lo ? key : lo;
    hi = key > hi ? key : hi;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long l2 = __shfl_xor(lo, o), h2 = __shfl_xor(hi, o);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
    nan |= __shfl_xor(nan, o);
  }
  if ((threadIdx.x & 63) == 0) {
    if (lo <= hi) {                          // the wave saw a number
      atomicMin(&p.ranges[2 * f], lo);
      atomicMax(&p.ranges[2 * f + 1], hi);
    }
    if (nan) atomicOr(&p.ranges[6], 1ull << f);
  }
}

// ---- 3. the frame ----
__device__ __forceinline__ int nearest_src(int dst, double ifx, int n) {
  const int s = (int)floor((double)dst * ifx);
  return s < n - 1 ? s : n - 1;
}

// entry of the colour map for field f at cell k: (x - min) / (max - min) in the field's own arithmetic, then matplotlib's
// `xa *= N; xa[xa == N] = N - 1; astype(int)`, NaN -> the bad colour (entry 256)
__device__ __forceinline__ int cmap_index(const VisEpP& p, int f, size_t k) {
#pragma clang fp contract(off)
  if ((p.ranges[6] >> f) & 1) return 256;
  const double mn = range_value(p.ranges[2 * f]), mx = range_value(p.ranges[2 * f + 1]);
  double scaled;
  if ((p.wide >> f) & 1) {
    const double x = ((p.wdata >> f) & 1) ? ((const double*)p.field[f])[k] : (double)((const float*)p.field[f])[k];
    scaled = ((x - mn) / (mx - mn)) * 256.0;
  } else {
    const float x = ((const float*)p.field[f])[k], fmn = (float)mn, fmx = (float)mx;
    scaled = (double)(((x - fmn) / (fmx - fmn)) * 256.0f);
  }
  if (scaled != scaled) return 256;
  // (a correctly rounded (x - min) / (max - min) lies in [0, 1]; the clamps are matplotlib's under / over colours and keep the index
  // inside the table whatever the field holds)
  return scaled >= 256.0 ? 255 : (scaled < 0.0 ? 0 : (int)scaled);
}

__device__ __forceinline__ unsigned cmap_bgr(const unsigned char* __restrict__ cmap, int idx) {
  return (unsigned)cmap[3 * idx] | ((unsigned)cmap[3 * idx + 1] << 8) | ((unsigned)cmap[3 * idx + 2] << 16);
}

// closed polygon, integer arithmetic: on an edge, or inside by crossing number
__device__ __forceinline__ bool in_arrow(const VisEpP& p, int x, int y) {
  bool inside = false;
  for (int a = 0; a < 4; ++a) {
    const int b = (a + 1) & 3;
    const long long x1 = p.ax[a], y1 = p.ay[a], x2 = p.ax[b], y2 = p.ay[b];
    const long long d = (x2 - x1) * (y - y1) - (x - x1) * (y2 - y1);
    if (d == 0 && x >= (x1 < x2 ? x1 : x2) && x <= (x1 < x2 ? x2 : x1) && y >= (y1 < y2 ? y1 : y2) && y <= (y1 < y2 ? y2 : y1)) return true;
    if ((y1 > y) != (y2 > y) && ((d > 0) == (y2 > y1))) inside = !inside;      // the edge crosses the ray to +x strictly right of x
  }
  return inside;
}

// the colour of frame pixel (y, x) as b | g << 8 | r << 16 where something lies over the background
__device__ __forceinline__ bool vis_pixel(const VisArgs& A, const VisEpP& p, int y, int x, unsigned* out) {
  if (x >= p.bx0 && x <= p.bx1 && y >= p.by0 && y <= p.by1 && in_arrow(p, x, y)) { *out = p.arrow_bgr; return true; }
  const bool pred = p.field[0] != nullptr;
  if (y >= 50 && y < 530) {
    if (x >= 15 && x < 655) {                                              // :556
      if (!p.rgb) return false;
      const unsigned char* s = p.rgb + ((size_t)(y - 50) * 640 + (x - 15)) * 3;
      *out = (unsigned)s[2] | ((unsigned)s[1] << 8) | ((unsigned)s[0] << 16);
      return true;
    }
    if (x >= 670 && x < 1150) {                                            // :545-557, :565-572
      const int m = A.m;
      const int i = m - 1 - nearest_src(y - 50, A.ifx_map, m), j = nearest_src(x - 670, A.ifx_map, m);      // flipud
      const unsigned char* c = A.palette + 3 * (int)p.index[(size_t)i * m + j];
      if (pred && (int)c[0] + c[1] + c[2] == 765) { *out = cmap_bgr(A.cmap, cmap_index(p, 0, (size_t)i * m + j)); return true; }
      *out = (unsigned)c[2] | ((unsigned)c[1] << 8) | ((unsigned)c[0] << 16);
      return true;
    }
    if (pred && x >= 1165 && x < 1405) {                                   // :575-587: dd_wt above, value below
      const int m = A.m, top = y < 290;
      const int i = m - 1 - nearest_src(y - (top ? 50 : 290), A.ifx_side, m), j = nearest_src(x - 1165, A.ifx_side, m);
      *out = cmap_bgr(A.cmap, cmap_index(p, top ? 2 : 1, (size_t)i * m + j));
      return true;
    }
  }
  if (pred && (((y == 49 || y == 530) && x >= 1165 && x < 1405) || (x == 1405 && y >= 49 && y < 531))) {      // :589-592
    *out = 100u | (100u << 8) | (100u << 16);
    return true;
  }
  return false;
}

__global__ __launch_bounds__(256) void vis_compose_kernel(const VisArgs A) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= V_CHUNKS) return;
  const VisEpP& p = A.p[blockIdx.y];
  const int b0 = t * 8;
  const uint2 bg = *(const uint2*)(A.background + b0);
  unsigned long long w = (unsigned long long)bg.x | ((unsigned long long)bg.y << 32);
  const int p0 = b0 / 3, p1 = (b0 + 7) / 3;
  for (int q = p0; q <= p1; ++q) {
    const int y = q / VW, x = q - y * VW;
    unsigned c;
    if (!vis_pixel(A, p, y, x, &c)) continue;
    for (int ch = 0; ch < 3; ++ch) {
      const int k = q * 3 + ch - b0;
      if (k >= 0 && k < 8) w = (w & ~(0xffull << (8 * k))) | ((unsigned long long)((c >> (8 * ch)) & 0xffu) << (8 * k));
    }
  }
  *(uint2*)(p.frame + b0) = make_uint2((unsigned)w, (unsigned)(w >> 32));
}

// ---- host ----
bool ranges_meet(uintptr_t a, size_t na, uintptr_t b, size_t nb) { return a < b + nb && b < a + na; }

// the checks of one episode and its packed arguments; `frame` false: peanut_vis_index_map
int vis_params(VisEpP& p, const peanut_vis_common_t* cm, const peanut_vis_episode_t* ep, bool frame, const std::string& who) {
  const int m = cm->m;
  if (!ep->local_map || !ep->collision_map || !ep->visited_vis || !ep->goal || !ep->index_map || !ep->ranges || (frame && !ep->frame))
    return fail(PEANUT_EINVAL, who + ": null pointer");
  if (ep->row_stride < m || ep->plane_stride < (long long)(m - 1) * ep->row_stride + m)
    return fail(PEANUT_EINVAL, who + ": strides under which planes or rows overlap");
  const int gx1 = ep->lmb[0], gx2 = ep->lmb[1], gy1 = ep->lmb[2], gy2 = ep->lmb[3];
  if (gx2 - gx1 != m || gy2 - gy1 != m || gx1 < 0 || gy1 < 0 || gx2 > cm->full_w || gy2 > cm->full_h)
    return fail(PEANUT_EINVAL, who + ": lmb is not an m x m window inside the full map");
  if (((uintptr_t)ep->ranges & 7) || (frame && ((uintptr_t)ep->frame & 7)))
    return fail(PEANUT_EINVAL, who + ": ranges and frame must be 8-byte aligned");
  p = VisEpP{};
  p.lm = ep->local_map; p.ps = ep->plane_stride; p.rs = ep->row_stride;
  p.collision = ep->collision_map + (size_t)gx1 * cm->full_h + gy1;
  p.visited = ep->visited_vis + (size_t)gx1 * cm->full_h + gy1;
  p.goal = ep->goal; p.rgb = ep->rgb; p.index = ep->index_map; p.ranges = (unsigned long long*)ep->ranges; p.frame = ep->frame;
  // `if int(stg[0]) < local_w and int(stg[1]) < local_h: sem_map[int(stg[0]), int(stg[1])] = 15` with NumPy's negative indices
  p.stg_r = p.stg_c = -1;
  if (ep->stg[0] < m && ep->stg[1] < m) {
    if (ep->stg[0] < -m || ep->stg[1] < -m) return fail(PEANUT_EINVAL, who + ": a stg coordinate below -m indexes outside the map");
    p.stg_r = ep->stg[0] < 0 ? ep->stg[0] + m : ep->stg[0];
    p.stg_c = ep->stg[1] < 0 ? ep->stg[1] + m : ep->stg[1];
  }
  p.bx0 = 1; p.bx1 = 0; p.by0 = 1; p.by1 = 0;
  if (!frame) return 0;
  if (ep->target_pred) {
    if (!ep->value || !ep->dd_wt) return fail(PEANUT_EINVAL, who + ": target_pred without value or dd_wt");
    p.field[0] = ep->target_pred; p.field[1] = ep->value; p.field[2] = ep->dd_wt;
    for (int f = 0; f < 3; ++f) {
      if ((ep->bits[f] != 32 && ep->bits[f] != 64) || (ep->data_bits[f] != 32 && ep->data_bits[f] != 64) || ep->bits[f] < ep->data_bits[f])
        return fail(PEANUT_EINVAL, who + ": bits and data_bits must be 32 or 64, bits not below data_bits");
      if (ep->bits[f] == 64) p.wide |= 1 << f;
      if (ep->data_bits[f] == 64) p.wdata |= 1 << f;
      if ((uintptr_t)p.field[f] & (ep->data_bits[f] == 64 ? 7 : 3)) return fail(PEANUT_EINVAL, who + ": a misaligned field");
    }
  }
  int x0 = INT32_MAX, x1 = INT32_MIN, y0 = INT32_MAX, y1 = INT32_MIN;
  for (int a = 0; a < 4; ++a) {
    const int x = ep->arrow[a][0], y = ep->arrow[a][1];
    if (x < -(1 << 20) || x > (1 << 20) || y < -(1 << 20) || y > (1 << 20)) return fail(PEANUT_EINVAL, who + ": an arrow vertex outside +-2^20");
    p.ax[a] = x; p.ay[a] = y;
    x0 = std::min(x0, x); x1 = std::max(x1, x); y0 = std::min(y0, y); y1 = std::max(y1, y);
  }
  p.bx0 = std::max(x0, 0); p.bx1 = std::min(x1, VW - 1); p.by0 = std::max(y0, 0); p.by1 = std::min(y1, VH - 1);
  p.arrow_bgr = (unsigned)ep->arrow_bgr[0] | ((unsigned)ep->arrow_bgr[1] << 8) | ((unsigned)ep->arrow_bgr[2] << 16);
  return 0;
}

int vis_launch(const peanut_vis_common_t* cm, int E, const peanut_vis_episode_t* eps, bool frame, const char* name) {
  const std::string who(name);
  if (!cm || !eps) return fail(PEANUT_EINVAL, who + ": null argument");
  if (E < 1 || E > PEANUT_VIS_MAX_BATCH) return fail(PEANUT_EINVAL, who + ": E must be 1..PEANUT_VIS_MAX_BATCH");
  const int m = cm->m;
  if (m < 1 || m > V_MAX_M || cm->channels < 5 || cm->channels > 260) return fail(PEANUT_EINVAL, who + ": m must be 1..4096, channels 5..260");
  if (!cm->palette || (frame && (!cm->background || !cm->cmap))) return fail(PEANUT_EINVAL, who + ": null table");
  if (frame && ((uintptr_t)cm->background & 7)) return fail(PEANUT_EINVAL, who + ": the background must be 8-byte aligned");
  if (cm->full_w < m || cm->full_h < m) return fail(PEANUT_EINVAL, who + ": the full map is smaller than the window");
  VisArgs A{};
  bool any_pred = false;
  const size_t nidx = (size_t)m * m, nrange = PEANUT_VIS_RANGE_WORDS * 8;
  for (int e = 0; e < E; ++e) {
    if (int rc = vis_params(A.p[e], cm, eps + e, frame, who)) return rc;
    any_pred = any_pred || eps[e].target_pred;
    for (int o = 0; o < e; ++o)
      if (ranges_meet((uintptr_t)eps[e].index_map, nidx, (uintptr_t)eps[o].index_map, nidx) ||
          ranges_meet((uintptr_t)eps[e].ranges, nrange, (uintptr_t)eps[o].ranges, nrange) ||
          (frame && ranges_meet((uintptr_t)eps[e].frame, V_BYTES, (uintptr_t)eps[o].frame, V_BYTES)))
        return fail(PEANUT_EINVAL, who + ": two episodes name the same output");
  }
  A.background = cm->background; A.palette = cm->palette; A.cmap = cm->cmap;
  A.m = m; A.ncat = cm->channels - 4; A.full_h = cm->full_h;
  A.ifx_map = 1.0 / (480.0 / (double)m);
  A.ifx_side = 1.0 / (240.0 / (double)m);
  hipStream_t s = (hipStream_t)cm->stream;
  hipLaunchKernelGGL(vis_index_kernel, dim3((m + V_TX - 1) / V_TX, (m + V_TY - 1) / V_TY, E), dim3(V_TX, V_TY), 0, s, A);
  if (frame) {
    if (any_pred) hipLaunchKernelGGL(vis_range_kernel, dim3(std::min(V_RANGE_BLOCKS, (m * m + 255) / 256), 3, E), dim3(256), 0, s, A);
    hipLaunchKernelGGL(vis_compose_kernel, dim3((V_CHUNKS + 255) / 256, E), dim3(256), 0, s, A);
  }
  hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : fail(PEANUT_EHIP, who + ": " + hipGetErrorString(err));
}

}  // namespace

}  // namespace peanut

using namespace peanut;

extern "C" int peanut_vis_index_map(const peanut_vis_common_t* common, const peanut_vis_episode_t* episode) {
  return vis_launch(common, 1, episode, false, "peanut_vis_index_map");
}

extern "C" int peanut_vis_render(const peanut_vis_common_t* common, const peanut_vis_episode_t* episode) {
  return vis_launch(common, 1, episode, true, "peanut_vis_render");
}

extern "C" int peanut_vis_render_batch(const peanut_vis_common_t* common, int E, const peanut_vis_episode_t* episodes) {
  return vis_launch(common, E, episodes, true, "peanut_vis_render_batch");
}

extern "C" int peanut_vis_sem_argmax(const peanut_vis_common_t* common, const float* local_map, long long plane_stride,
                                     long long row_stride, uint8_t* out) {
  if (!common || !local_map || !out) return fail(PEANUT_EINVAL, "peanut_vis_sem_argmax: null pointer");
  const int channels = common->channels, m = common->m;
  if (channels < 5 || channels > 260 || m < 1 || m > V_MAX_M || row_stride < m || plane_stride < (long long)(m - 1) * row_stride + m)
    return fail(PEANUT_EINVAL, "peanut_vis_sem_argmax: bad dimensions or strides");
  hipLaunchKernelGGL(vis_sem_argmax_kernel, dim3((m * m + 255) / 256), dim3(256), 0, (hipStream_t)common->stream, local_map,
                     plane_stride, row_stride, channels - 4, m, out);
  hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : fail(PEANUT_EHIP, std::string("peanut_vis_sem_argmax: ") + hipGetErrorString(err));
}
