// Sliding-window and flip-averaged inference of the map-prediction model (ABI 24): the paths of the reference's EncoderDecoder
// around its forward -- slide_inference (prediction/mmseg/models/segmentors/encoder_decoder.py:155-201), the flip branch of
// inference() (:249-256) and the averaging of aug_test (:273-291) -- as two HBM-bound launches around ONE batched forward:
//
//   infer_gather_kernel    every window of every (flipped) image into one staged batch [N, C, ch, cw]
//   (the forward, raw logits at window resolution, csrc/pred_api.hip)
//   infer_combine_kernel   window sums / counts, un-flip, the mean over the augmentations, the optional sigmoid -> [B, K, H, W]
//
// The window grid is host arithmetic (infer_grid: the reference's loop, :166-177) and travels by value in the kernel arguments.
// Plain HIP: loads, fp32 adds and IEEE divisions; no atomics, no LDS.
#include <algorithm>

#include "net_common.h"

namespace peanut {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocksX = 2048;     // per staged map / in all: the rest of the work is a grid-stride loop
constexpr int kMaxBlocksY = 4096;

struct InferArgs {                    // by value
  int n_augs, B, C, H, W;             // C: channels of what the kernel moves (gather: input channels, combine: classes)
  int ch, cw, ny, nx;
  int slide, sigmoid;
  int flip[PEANUT_INFER_MAX_AUGS];
  int y1[PEANUT_INFER_MAX_GRID], x1[PEANUT_INFER_MAX_GRID];
};

// staged[n][c][r][j] = F_a(in[b])[c][y1[wy] + r][x1[wx] + j] with n = (a * B + b) * ny * nx + wy * nx + wx: the flip F_a is applied to
// the whole image before the windows are cut (np.flip in the pipeline's RandomFlip).  A thread moves four x-neighbours: VEC with
// 16-byte accesses (W, cw and every x1 multiples of 4, both pointers 16-byte aligned; a horizontally flipped group is one aligned
// group of the source read reversed), else element by element.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void infer_gather_kernel(const float* __restrict__ in, float* __restrict__ staged, const InferArgs A) {
  const int nwin = A.ny * A.nx, N = A.n_augs * A.B * nwin;
  const int cw4 = (A.cw + 3) / 4;
  const long long items = (long long)A.C * A.ch * cw4;
  for (int n = blockIdx.y; n < N; n += gridDim.y) {
    const int win = n % nwin, ab = n / nwin;
    const int b = ab % A.B, a = ab / A.B;
    const int wy = win / A.nx, wx = win - wy * A.nx;
    const int y0 = A.y1[wy], x0 = A.x1[wx], f = A.flip[a];
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < items; i += (long long)gridDim.x * kThreads) {
      const long long row = i / cw4;
      const int j = (int)(i - row * cw4) * 4;
      const int c = (int)(row / A.ch), r = (int)(row - (long long)c * A.ch);
      const int y = y0 + r, x = x0 + j;                       // in the flipped image
      const int ys = f == 2 ? A.H - 1 - y : y;
      const float* p = in + (((long long)b * A.C + c) * A.H + ys) * A.W;
      float* q = staged + (((long long)n * A.C + c) * A.ch + r) * A.cw + j;
      if (VEC) {
        float4 v;
        if (f == 1) {
          const float4 u = *reinterpret_cast<const float4*>(p + (A.W - 4 - x));
          v.x = u.w; v.y = u.z; v.z = u.y; v.w = u.x;
        } else {
          v = *reinterpret_cast<const float4*>(p + x);
        }
        *reinterpret_cast<float4*>(q) = v;
      } else {
        const int m = A.cw - j;                               // >= 1
        const int step = f == 1 ? -1 : 1;
        const float* ps = p + (f == 1 ? A.W - 1 - x : x);
        q[0] = ps[0];
        if (m > 1) q[1] = ps[step];
        if (m > 2) q[2] = ps[2 * step];
        if (m > 3) q[3] = ps[3 * step];
      }
    }
  }
}

// out[b][k][y][x], the rule of include/peanut_hip.h in its order.  Per augmentation a, at the pixel's place (yf, xf) in the flipped
// image: s = +0.0f; s = s + logit for every covering window in row-major order; p = s / (float)count (slide) or the one logit
// (whole); then out = p_0, out = out + p_a, out = out / (float)n_augs if n_augs > 1, the optional sigmoid.  V = 4: a thread holds
// four x-neighbours (W, cw and every x1 multiples of 4: an aligned group lies inside a window or outside it as a whole; under a
// horizontal flip it is one aligned group of the flipped image, reversed), V = 1 otherwise.
template <int V>
__global__ __launch_bounds__(kThreads) void infer_combine_kernel(const float* __restrict__ logits, float* __restrict__ out, const InferArgs A) {
  const int nwin = A.ny * A.nx;
  const int Wg = A.W / V;
  const long long total = (long long)A.B * A.C * A.H * Wg;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kThreads) {
    const int x = (int)(i % Wg) * V;
    long long t = i / Wg;
    const int y = (int)(t % A.H);
    t /= A.H;
    const int k = (int)(t % A.C), b = (int)(t / A.C);
    float acc[V];
    for (int a = 0; a < A.n_augs; ++a) {
      const int f = A.flip[a];
      const int yf = f == 2 ? A.H - 1 - y : y;
      const int xf = f == 1 ? A.W - V - x : x;
      const long long n0 = (long long)(a * A.B + b) * nwin;
      float s[V], v[V];
      int cnt = 0;
#pragma unroll
      for (int q = 0; q < V; ++q) s[q] = 0.0f, v[q] = 0.0f;
      for (int wy = 0; wy < A.ny; ++wy) {
        const int ry = yf - A.y1[wy];
        if ((unsigned)ry >= (unsigned)A.ch) continue;
        for (int wx = 0; wx < A.nx; ++wx) {
          const int rx = xf - A.x1[wx];
          if ((unsigned)rx >= (unsigned)A.cw) continue;
          const float* p = logits + (((n0 + wy * A.nx + wx) * A.C + k) * A.ch + ry) * A.cw + rx;
          if (V == 4) {
            const float4 u = *reinterpret_cast<const float4*>(p);
            v[0] = u.x; v[V > 1 ? 1 : 0] = u.y; v[V > 2 ? 2 : 0] = u.z; v[V > 3 ? 3 : 0] = u.w;
          } else {
            v[0] = p[0];
          }
#pragma unroll
          for (int q = 0; q < V; ++q) s[q] = s[q] + v[q];
          ++cnt;
        }
      }
      const float fc = (float)cnt;
#pragma unroll
      for (int q = 0; q < V; ++q) {
        const float p = A.slide ? s[q] / fc : v[q];
        const int o = f == 1 ? V - 1 - q : q;                 // un-flip inside the group
        acc[o] = a == 0 ? p : acc[o] + p;
      }
    }
    if (A.n_augs > 1) {
      const float fa = (float)A.n_augs;
#pragma unroll
      for (int q = 0; q < V; ++q) acc[q] = acc[q] / fa;
    }
    if (A.sigmoid) {
#pragma unroll
      for (int q = 0; q < V; ++q) acc[q] = 1.f / (1.f + expf(-acc[q]));
    }
    float* o = out + (((long long)b * A.C + k) * A.H + y) * A.W + x;
    if (V == 4) {
      float4 u;
      u.x = acc[0]; u.y = acc[V > 1 ? 1 : 0]; u.z = acc[V > 2 ? 2 : 0]; u.w = acc[V > 3 ? 3 : 0];
      *reinterpret_cast<float4*>(o) = u;
    } else {
      o[0] = acc[0];
    }
  }
}

InferArgs make_args(const InferGrid& g, int slide, int n_augs, const int* flip, int B, int C, int H, int W, int sigmoid) {
  InferArgs A{};
  A.n_augs = n_augs; A.B = B; A.C = C; A.H = H; A.W = W;
  A.ch = g.ch; A.cw = g.cw; A.ny = g.ny; A.nx = g.nx;
  A.slide = slide; A.sigmoid = sigmoid;
  for (int a = 0; a < n_augs; ++a) A.flip[a] = flip[a];
  for (int i = 0; i < g.ny; ++i) A.y1[i] = g.y1[i];
  for (int i = 0; i < g.nx; ++i) A.x1[i] = g.x1[i];
  return A;
}

// 16-byte accesses: every row of the image and of a window starts on a multiple of four floats, and so does every window
bool vector_ok(const InferGrid& g, int W, const void* a, const void* b) {
  bool ok = W % 4 == 0 && g.cw % 4 == 0 && (uintptr_t)a % 16 == 0 && (uintptr_t)b % 16 == 0;
  for (int i = 0; i < g.nx && ok; ++i) ok = g.x1[i] % 4 == 0;
  return ok;
}

int blocks_for(long long items, int cap) {
  return (int)std::min<long long>(std::max<long long>((items + kThreads - 1) / kThreads, 1), cap);
}

// One axis of slide_inference's loop (:166-177): grids = max(n - crop + stride - 1, 0) // stride + 1 windows, window i ends at
// min(i * stride + crop, n) and starts at max(end - crop, 0).  Returns the count (0: more than PEANUT_INFER_MAX_GRID).
int axis_windows(int n, int crop, int stride, int* start) {
  const long long grids = std::max<long long>((long long)n - crop + stride - 1, 0) / stride + 1;
  if (grids > PEANUT_INFER_MAX_GRID) return 0;
  for (int i = 0; i < (int)grids; ++i) {
    const long long end = std::min<long long>((long long)i * stride + crop, n);
    start[i] = (int)std::max<long long>(end - crop, 0);
  }
  return (int)grids;
}

// true when consecutive windows of `size` leave no cell of the axis out (the first starts at 0 and the last ends at n by construction)
bool axis_covered(const int* start, int count, int size) {
  for (int i = 0; i + 1 < count; ++i)
    if (start[i + 1] > start[i] + size) return false;
  return true;
}

}  // namespace

int infer_grid(const peanut_pred_infer_t* d, int H, int W, InferGrid* g, const char* who) {
  const std::string w(who);
  if (!d || !g) return fail(PEANUT_EINVAL, w + ": null argument");
  if (d->mode != 0 && d->mode != 1) return fail(PEANUT_EINVAL, w + ": mode must be 0 (whole) or 1 (slide)");
  if (d->n_augs < 1 || d->n_augs > PEANUT_INFER_MAX_AUGS) return fail(PEANUT_EINVAL, w + ": n_augs must be 1..PEANUT_INFER_MAX_AUGS");
  for (int a = 0; a < d->n_augs; ++a)
    if (d->flip[a] < 0 || d->flip[a] > 2) return fail(PEANUT_EINVAL, w + ": a flip code must be 0 (none), 1 (horizontal) or 2 (vertical)");
  if (d->max_batch < 0) return fail(PEANUT_EINVAL, w + ": max_batch must be >= 0");
  if (H < 1 || W < 1) return fail(PEANUT_EINVAL, w + ": the image must be at least 1 x 1");
  *g = InferGrid{};
  if (d->mode == 0) {
    g->ny = g->nx = 1;
    g->ch = H; g->cw = W;
  } else {
    if (d->crop_h < 1 || d->crop_w < 1 || d->stride_h < 1 || d->stride_w < 1)
      return fail(PEANUT_EINVAL, w + ": slide mode needs crop_size and stride >= 1");
    g->ny = axis_windows(H, d->crop_h, d->stride_h, g->y1);
    g->nx = axis_windows(W, d->crop_w, d->stride_w, g->x1);
    if (!g->ny || !g->nx) return fail(PEANUT_EINVAL, w + ": more than PEANUT_INFER_MAX_GRID windows on an axis");
    g->ch = std::min(d->crop_h, H); g->cw = std::min(d->crop_w, W);
    if (!axis_covered(g->y1, g->ny, g->ch) || !axis_covered(g->x1, g->nx, g->cw))
      return fail(PEANUT_EINVAL, w + ": a pixel that no window covers (stride > crop_size; the reference asserts on it)");
  }
  if (g->ch < 16 || g->cw < 16) return fail(PEANUT_EINVAL, w + ": the forward needs windows of at least 16 x 16");
  return 0;
}

int launch_infer_gather(const float* in, float* staged, const InferGrid& g, int n_augs, const int* flip, int B, int C, int H, int W,
                        hipStream_t s) {
  const InferArgs A = make_args(g, 0, n_augs, flip, B, C, H, W, 0);
  const long long N = (long long)n_augs * B * g.ny * g.nx;
  const dim3 grid(blocks_for((long long)C * g.ch * ((g.cw + 3) / 4), kMaxBlocksX), (unsigned)std::min<long long>(N, kMaxBlocksY));
  if (vector_ok(g, W, in, staged)) infer_gather_kernel<true><<<grid, kThreads, 0, s>>>(in, staged, A);
  else infer_gather_kernel<false><<<grid, kThreads, 0, s>>>(in, staged, A);
  PEANUT_HIP_CHECK(hipGetLastError());
  return 0;
}

int launch_infer_combine(const float* logits, float* out, const InferGrid& g, int slide, int n_augs, const int* flip, int B, int K,
                         int H, int W, int sigmoid, hipStream_t s) {
  const InferArgs A = make_args(g, slide, n_augs, flip, B, K, H, W, sigmoid);
  if (vector_ok(g, W, logits, out))
    infer_combine_kernel<4><<<blocks_for((long long)B * K * H * (W / 4), 8 * kMaxBlocksX), kThreads, 0, s>>>(logits, out, A);
  else
    infer_combine_kernel<1><<<blocks_for((long long)B * K * H * W, 8 * kMaxBlocksX), kThreads, 0, s>>>(logits, out, A);
  PEANUT_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace peanut

using namespace peanut;

extern "C" {

int peanut_pred_infer_windows(const peanut_pred_infer_t* infer, int H, int W, int* y1, int* x1, int* ch, int* cw) {
  InferGrid g;
  if (int rc = infer_grid(infer, H, W, &g, "peanut_pred_infer_windows")) return rc;
  for (int i = 0; i < PEANUT_INFER_MAX_GRID; ++i) {
    if (y1) y1[i] = i < g.ny ? g.y1[i] : -1;
    if (x1) x1[i] = i < g.nx ? g.x1[i] : -1;
  }
  if (ch) *ch = g.ch;
  if (cw) *cw = g.cw;
  return g.ny * g.nx;
}

namespace {
bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}
}  // namespace

int peanut_pred_infer_gather(const peanut_pred_infer_t* infer, const float* in_dev, float* staged_dev, int B, int C, int H, int W) {
  InferGrid g;
  if (int rc = infer_grid(infer, H, W, &g, "peanut_pred_infer_gather")) return rc;
  if (!in_dev || !staged_dev || B < 1 || C < 1) return fail(PEANUT_EINVAL, "peanut_pred_infer_gather: null pointer, or B or C below 1");
  const long long N = (long long)infer->n_augs * B * g.ny * g.nx;
  if (N > (1 << 20)) return fail(PEANUT_EINVAL, "peanut_pred_infer_gather: more than 2^20 staged windows");
  if (overlaps(in_dev, (size_t)B * C * H * W * sizeof(float), staged_dev, (size_t)N * C * g.ch * g.cw * sizeof(float)))
    return fail(PEANUT_EINVAL, "peanut_pred_infer_gather: staged_dev overlaps in_dev");
  return launch_infer_gather(in_dev, staged_dev, g, infer->n_augs, infer->flip, B, C, H, W, (hipStream_t)infer->stream);
}

int peanut_pred_infer_combine(const peanut_pred_infer_t* infer, const float* logits_dev, float* out_dev, int B, int K, int H, int W,
                              int apply_sigmoid) {
  InferGrid g;
  if (int rc = infer_grid(infer, H, W, &g, "peanut_pred_infer_combine")) return rc;
  if (!logits_dev || !out_dev || B < 1 || K < 1) return fail(PEANUT_EINVAL, "peanut_pred_infer_combine: null pointer, or B or K below 1");
  const long long N = (long long)infer->n_augs * B * g.ny * g.nx;
  if (N > (1 << 20)) return fail(PEANUT_EINVAL, "peanut_pred_infer_combine: more than 2^20 staged windows");
  if (overlaps(logits_dev, (size_t)N * K * g.ch * g.cw * sizeof(float), out_dev, (size_t)B * K * H * W * sizeof(float)))
    return fail(PEANUT_EINVAL, "peanut_pred_infer_combine: out_dev overlaps logits_dev");
  return launch_infer_combine(logits_dev, out_dev, g, infer->mode, infer->n_augs, infer->flip, B, K, H, W, apply_sigmoid,
                              (hipStream_t)infer->stream);
}

}  // extern "C"
