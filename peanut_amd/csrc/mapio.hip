// Map datasets on the device (ABI 21): the snapshots nav/collect_maps.py takes of the full map, the model inputs
// prediction/train_prediction_model.py makes of a stored sequence, and the loss it trains with -- all on uint8 sequences that
// stay in device memory.  Three HBM-bound kernels and one small finish kernel; plain HIP, integer atomics only.
// ABI 25 adds the training side: the reference's train_pipeline (pad, random crop, flip, rotation) of a batch of samples as one
// gather, input and target, and the loss against such a stored target.
#include <algorithm>
#include <cmath>
#include <mutex>

#include "net_common.h"

namespace peanut {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;      // per episode / sample: the rest of the work is a grid-stride loop

// Sum of one value per thread over a workgroup of kThreads, as a fixed tree over the thread index (the same order in every
// launch: the double sums of the loss must not depend on the run).  `sh` holds kThreads values; every thread gets the sum.
template <class T>
__device__ __forceinline__ T block_sum(T v, T* sh) {
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
#pragma unroll
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (tid < s) sh[tid] += sh[tid + s];
    __syncthreads();
  }
  const T r = sh[0];
  __syncthreads();
  return r;
}

// ---- 1. snapshots: uint8(full_map * 255) of up to PEANUT_MAPSEQ_MAX_BATCH episodes, with the two sums of the dataset filter ----
struct EncodeArgs {
  const float* src[PEANUT_MAPSEQ_MAX_BATCH];      // by value: every episode owns its map
  unsigned char* dst[PEANUT_MAPSEQ_MAX_BATCH];
  long long plane_stride[PEANUT_MAPSEQ_MAX_BATCH], row_stride[PEANUT_MAPSEQ_MAX_BATCH];   // floats
  unsigned vec_mask;                               // bit e: every row of episode e takes 16-byte loads and 4-byte stores
  int C, W, H, H4;                                 // H4 = ceil(H / 4): a thread's item is four cells of one row
  unsigned long long* sums;                        // [E][2]: bytes of channels 4:, bytes of channel 1
};

// One multiply, then truncation: numpy's `(x * 255).astype(np.uint8)` on [0, 256/255).  Everything else saturates (NaN -> 0).
__device__ __forceinline__ unsigned encode_byte(float x) {
  return (unsigned)fminf(fmaxf(x * 255.0f, 0.0f), 255.0f);
}

__global__ __launch_bounds__(kThreads) void mapseq_encode_kernel(const EncodeArgs A) {
  __shared__ unsigned long long sh[kThreads];
  const int e = blockIdx.y;
  const float* __restrict__ src = A.src[e];
  unsigned char* __restrict__ dst = A.dst[e];
  const long long ps = A.plane_stride[e], rs = A.row_stride[e];
  const bool vec = (A.vec_mask >> e) & 1u;
  const long long items = (long long)A.C * A.W * A.H4;
  unsigned long long s_sem = 0, s_exp = 0;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < items; i += (long long)gridDim.x * kThreads) {
    const long long row = i / A.H4;
    const int h = (int)(i - row * A.H4) * 4;
    const int c = (int)(row / A.W), w = (int)(row - (long long)c * A.W);
    const float* p = src + c * ps + w * rs + h;
    unsigned char* q = dst + row * A.H + h;
    unsigned b0, b1 = 0, b2 = 0, b3 = 0;
    if (vec) {
      const float4 v = *reinterpret_cast<const float4*>(p);
      b0 = encode_byte(v.x); b1 = encode_byte(v.y); b2 = encode_byte(v.z); b3 = encode_byte(v.w);
      *reinterpret_cast<unsigned*>(q) = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
    } else {
      const int n = A.H - h;                       // >= 1
      b0 = encode_byte(p[0]); q[0] = (unsigned char)b0;
      if (n > 1) { b1 = encode_byte(p[1]); q[1] = (unsigned char)b1; }
      if (n > 2) { b2 = encode_byte(p[2]); q[2] = (unsigned char)b2; }
      if (n > 3) { b3 = encode_byte(p[3]); q[3] = (unsigned char)b3; }
    }
    const unsigned s = b0 + b1 + b2 + b3;
    if (c == 1) s_exp += s;
    else if (c >= 4) s_sem += s;
  }
  s_sem = block_sum(s_sem, sh);
  s_exp = block_sum(s_exp, sh);
  if (threadIdx.x == 0) {                          // exact integers: the order of the adds does not matter
    if (s_sem) atomicAdd(A.sums + 2 * e, s_sem);
    if (s_exp) atomicAdd(A.sums + 2 * e + 1, s_exp);
  }
}

// ---- 2. / 3. the samples of a stored sequence ----
struct SampleArgs {                                // by value
  int t[PEANUT_MAPSEQ_MAX_SAMPLES], x1[PEANUT_MAPSEQ_MAX_SAMPLES], y1[PEANUT_MAPSEQ_MAX_SAMPLES];
};

// out[b][c][i][j] = float(maps[t_b][c][x1_b + i][y1_b + j]) / 255.0f (an IEEE division: np.float32(k) / np.float32(255))
template <bool VEC>
__global__ __launch_bounds__(kThreads) void mapseq_inputs_kernel(const unsigned char* __restrict__ maps, int C, int W, int H, const SampleArgs P,
                                                                 int S, int S4, float* __restrict__ out) {
  const int b = blockIdx.y;
  const int t = P.t[b], x1 = P.x1[b], y1 = P.y1[b];
  const long long items = (long long)C * S * S4;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < items; i += (long long)gridDim.x * kThreads) {
    const long long row = i / S4;
    const int j = (int)(i - row * S4) * 4;
    const int c = (int)(row / S), r = (int)(row - (long long)c * S);
    const unsigned char* p = maps + (((long long)t * C + c) * W + (x1 + r)) * H + (y1 + j);
    float* q = out + (((long long)b * C + c) * S + r) * S + j;
    if (VEC) {
      const unsigned v = *reinterpret_cast<const unsigned*>(p);
      float4 o;
      o.x = (float)(v & 255u) / 255.0f; o.y = (float)((v >> 8) & 255u) / 255.0f;
      o.z = (float)((v >> 16) & 255u) / 255.0f; o.w = (float)(v >> 24) / 255.0f;
      *reinterpret_cast<float4*>(q) = o;
    } else {
      const int n = S - j;
      q[0] = (float)p[0] / 255.0f;
      if (n > 1) q[1] = (float)p[1] / 255.0f;
      if (n > 2) q[2] = (float)p[2] / 255.0f;
      if (n > 3) q[3] = (float)p[3] / 255.0f;
    }
  }
}

constexpr int kBceCells = 4 * kThreads;            // cells of one workgroup's chunk: THE partition of a window, a function of S alone

// partial[(b * K + k) * nchunks + chunk] = sum over the chunk's cells of the loss of channel k, in double.  A thread holds four
// cells kThreads apart, reads their explored bytes once and walks the K channels; its four terms are added in cell order, the
// workgroup's 256 sums by block_sum's tree.
__global__ __launch_bounds__(kThreads) void mapseq_bce_kernel(const unsigned char* __restrict__ maps, int T, int C, int W, int H, const SampleArgs P,
                                                              int S, const float* __restrict__ logits, int K, double* __restrict__ partial,
                                                              int nchunks) {
  __shared__ double sh[kThreads];
  const int b = blockIdx.y, chunk = blockIdx.x;
  const int cells = S * S;
  const long long plane = (long long)W * H;
  const unsigned char* expl = maps + ((long long)P.t[b] * C + 1) * plane;
  const unsigned char* tgt = maps + ((long long)(T - 1) * C + 4) * plane;
  const int x1 = P.x1[b], y1 = P.y1[b];
  int cell[4], off[4];
  bool open[4];                                    // inside the window and unexplored at t_idx: the target byte counts
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    cell[r] = chunk * kBceCells + r * kThreads + (int)threadIdx.x;
    const bool valid = cell[r] < cells;
    const int i = valid ? cell[r] / S : 0, j = valid ? cell[r] - i * S : 0;
    off[r] = (x1 + i) * H + (y1 + j);
    open[r] = valid && expl[off[r]] == 0;
    if (!valid) cell[r] = -1;
  }
  for (int k = 0; k < K; ++k) {
    const float* lg = logits + ((long long)b * K + k) * cells;
    const unsigned char* tk = tgt + k * plane;
    double acc = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (cell[r] < 0) continue;
      const unsigned byte = open[r] ? tk[off[r]] : 0u;
      const double x = (double)lg[cell[r]];
      const double y = (double)((float)byte / 255.0f);
      acc += (1.0 - y) * x + fmax(-x, 0.0) + log1p(exp(-fabs(x)));
    }
    const double tot = block_sum(acc, sh);
    if (threadIdx.x == 0) partial[((long long)b * K + k) * nchunks + chunk] = tot;
  }
}

// sum[bk] = the nchunks partials of (b, k): thread l adds chunks l, l + 256, ... in index order, then block_sum's tree
__global__ __launch_bounds__(kThreads) void mapseq_bce_finish_kernel(const double* __restrict__ partial, int nchunks, double* __restrict__ sum) {
  __shared__ double sh[kThreads];
  const double* p = partial + (long long)blockIdx.x * nchunks;
  double acc = 0.0;
  for (int c = threadIdx.x; c < nchunks; c += kThreads) acc += p[c];
  const double tot = block_sum(acc, sh);
  if (threadIdx.x == 0) sum[blockIdx.x] = tot;
}

// The same against a stored target (peanut_mapseq_bce_dense): gt[(b * K + k) * cells + cell] is the byte.  The cell formula, the
// partition and the order of the adds are those of mapseq_bce_kernel, so that equal target bytes give equal bits.
__global__ __launch_bounds__(kThreads) void mapseq_bce_dense_kernel(const unsigned char* __restrict__ gt, int cells, const float* __restrict__ logits,
                                                                    int K, double* __restrict__ partial, int nchunks) {
  __shared__ double sh[kThreads];
  const int b = blockIdx.y, chunk = blockIdx.x;
  int cell[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    cell[r] = chunk * kBceCells + r * kThreads + (int)threadIdx.x;
    if (cell[r] >= cells) cell[r] = -1;
  }
  for (int k = 0; k < K; ++k) {
    const float* lg = logits + ((long long)b * K + k) * cells;
    const unsigned char* tk = gt + ((long long)b * K + k) * cells;
    double acc = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (cell[r] < 0) continue;
      const unsigned byte = tk[cell[r]];
      const double x = (double)lg[cell[r]];
      const double y = (double)((float)byte / 255.0f);
      acc += (1.0 - y) * x + fmax(-x, 0.0) + log1p(exp(-fabs(x)));
    }
    const double tot = block_sum(acc, sh);
    if (threadIdx.x == 0) partial[((long long)b * K + k) * nchunks + chunk] = tot;
  }
}

// ---- 4. augmented training batches: pad, crop, flip and rotation of a sample as one gather ----
constexpr int kTileRows = 16, kTileCols = 64;      // a workgroup's tile of the crop: 16 rows of 16 threads with four cells each

struct TrainSample {                               // peanut_mapseq_aug_t as the kernel reads it (48 bytes)
  const unsigned char* maps;
  int T, t, oh, ow, flip, rotate;
  double c, s;
};
struct TrainArgs {                                 // by value: 3 KiB of samples and the shared sizes
  TrainSample smp[PEANUT_MAPSEQ_MAX_SAMPLES];
  int C, W, H, Sr, Sc, K;
  int vec_img, vec_gt;                             // 16-byte image stores / 4-byte target stores: S_c % 4 == 0 and an aligned base
  float* img;
  unsigned char* gt;                               // may be null
};

// Offset in a source plane of the cell behind cell (yi, xi) of the flipped crop; -1 where the rule gives zero (outside the crop:
// the constant border; beyond the map: the padding at the bottom and right).
__device__ __forceinline__ int tap_offset(int yi, int xi, int Sr, int Sc, int flip, int oh, int ow, int W, int H) {
  if ((unsigned)yi >= (unsigned)Sr || (unsigned)xi >= (unsigned)Sc) return -1;
  if (flip == 1) xi = Sc - 1 - xi;
  else if (flip == 2) yi = Sr - 1 - yi;
  const int r = yi + oh, q = xi + ow;
  return (r < W && q < H) ? r * H + q : -1;
}

// Four bytes of a plane, byte i the one behind off[i] (0 where off[i] < 0).  `run`: the four cells are valid and lie side by side
// from `lo` on, backwards when `rev`; they come as one 4-byte load where the address allows it.
__device__ __forceinline__ unsigned load_four(const unsigned char* __restrict__ pl, bool run, int lo, bool rev, const int (&off)[4]) {
  if (run && (reinterpret_cast<uintptr_t>(pl + lo) & 3u) == 0) {
    const unsigned v = *reinterpret_cast<const unsigned*>(pl + lo);
    return rev ? __builtin_bswap32(v) : v;
  }
  unsigned v = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (off[i] >= 0) v |= (unsigned)pl[off[i]] << (8 * i);
  return v;
}

__device__ __forceinline__ void store_img(float* q, const float (&o)[4], int n, bool vec) {
  if (vec) {
    *reinterpret_cast<float4*>(q) = make_float4(o[0], o[1], o[2], o[3]);
  } else {
    q[0] = o[0];
    if (n > 1) q[1] = o[1];
    if (n > 2) q[2] = o[2];
    if (n > 3) q[3] = o[3];
  }
}

__device__ __forceinline__ void store_gt(unsigned char* q, unsigned v, int n, bool vec) {
  if (vec) {
    *reinterpret_cast<unsigned*>(q) = v;
  } else {
    q[0] = (unsigned char)(v & 255u);
    if (n > 1) q[1] = (unsigned char)((v >> 8) & 255u);
    if (n > 2) q[2] = (unsigned char)((v >> 16) & 255u);
    if (n > 3) q[3] = (unsigned char)(v >> 24);
  }
}

// grid (ceil(S_c / 64), ceil(S_r / 16), B).  The coordinates, taps and weights of a thread's four cells are formed once and
// reused over the C image planes, the explored plane and the K target planes.  lut[k] = float(k) / 255.0f, the IEEE division,
// made once per workgroup: a tap is a byte load and an LDS read.
__global__ __launch_bounds__(kThreads) void mapseq_train_kernel(const TrainArgs A) {
  __shared__ float lut[kThreads];
  lut[threadIdx.x] = (float)threadIdx.x / 255.0f;
  __syncthreads();
  const TrainSample& P = A.smp[blockIdx.z];
  const int b = blockIdx.z;
  const int Sr = A.Sr, Sc = A.Sc, W = A.W, H = A.H, C = A.C, K = A.K;
  const int y = blockIdx.y * kTileRows + (int)(threadIdx.x >> 4);
  const int x0 = blockIdx.x * kTileCols + (int)(threadIdx.x & 15u) * 4;
  if (y >= Sr || x0 >= Sc) return;
  const int n = min(4, Sc - x0);                   // cells of this thread
  const int flip = P.flip, oh = P.oh, ow = P.ow;
  const long long plane = (long long)W * H;
  const unsigned char* __restrict__ snap = P.maps + (long long)P.t * C * plane;            // snapshot t_idx
  const unsigned char* __restrict__ last = P.maps + ((long long)(P.T - 1) * C + 4) * plane; // the target planes
  const long long cells = (long long)Sr * Sc;
  float* __restrict__ img = A.img + (long long)b * C * cells + (long long)y * Sc + x0;
  unsigned char* __restrict__ gt = A.gt ? A.gt + (long long)b * K * cells + (long long)y * Sc + x0 : nullptr;
  const bool vec_img = A.vec_img != 0, vec_gt = A.vec_gt != 0;

  if (!P.rotate) {
    int off[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) off[i] = i < n ? tap_offset(y, x0 + i, Sr, Sc, flip, oh, ow, W, H) : -1;
    const bool rev = flip == 1;
    const int lo = rev ? off[3] : off[0];
    const bool run = off[0] >= 0 && off[3] >= 0;   // one row, both ends inside the map: the four lie side by side
    for (int c = 0; c < C; ++c) {
      const unsigned v = load_four(snap + c * plane, run, lo, rev, off);
      const float o[4] = {lut[v & 255u], lut[(v >> 8) & 255u], lut[(v >> 16) & 255u], lut[v >> 24]};
      store_img(img + c * cells, o, n, vec_img);
    }
    if (gt) {
      const unsigned e = load_four(snap + plane, run, lo, rev, off);
      unsigned open = 0;                           // 0xff per unexplored cell (a zero tap stays zero either way)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (((e >> (8 * i)) & 255u) == 0) open |= 255u << (8 * i);
      for (int k = 0; k < K; ++k) store_gt(gt + k * cells, load_four(last + k * plane, run, lo, rev, off) & open, n, vec_gt);
    }
    return;
  }

  const double cy = 0.5 * (Sr - 1), cx = 0.5 * (Sc - 1);
  const double cs = P.c, sn = P.s;
  int off[4][4], near[4];
  float wt[4][4];
  const double dy = (double)y - cy;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double dx = (double)(x0 + i) - cx;
    const double ys = cs * dy - sn * dx + cy, xs = sn * dy + cs * dx + cx;
    // clamped before the conversion: -2 and S stand for every row / column whose two taps lie outside the crop
    const double y0 = fmin(fmax(floor(ys), -2.0), (double)Sr), x0f = fmin(fmax(floor(xs), -2.0), (double)Sc);
    const double fy = ys - floor(ys), fx = xs - floor(xs);
    const int iy = (int)y0, ix = (int)x0f;
    const bool mine = i < n;
    off[i][0] = mine ? tap_offset(iy, ix, Sr, Sc, flip, oh, ow, W, H) : -1;
    off[i][1] = mine ? tap_offset(iy, ix + 1, Sr, Sc, flip, oh, ow, W, H) : -1;
    off[i][2] = mine ? tap_offset(iy + 1, ix, Sr, Sc, flip, oh, ow, W, H) : -1;
    off[i][3] = mine ? tap_offset(iy + 1, ix + 1, Sr, Sc, flip, oh, ow, W, H) : -1;
    wt[i][0] = (float)((1.0 - fy) * (1.0 - fx));
    wt[i][1] = (float)((1.0 - fy) * fx);
    wt[i][2] = (float)(fy * (1.0 - fx));
    wt[i][3] = (float)(fy * fx);
    const double yn = fmin(fmax(floor(ys + 0.5), -1.0), (double)Sr), xn = fmin(fmax(floor(xs + 0.5), -1.0), (double)Sc);
    near[i] = mine ? tap_offset((int)yn, (int)xn, Sr, Sc, flip, oh, ow, W, H) : -1;
  }
  for (int c = 0; c < C; ++c) {
    const unsigned char* __restrict__ pl = snap + c * plane;
    float o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float v = wt[i][0] * (off[i][0] >= 0 ? lut[pl[off[i][0]]] : 0.0f);
      v += wt[i][1] * (off[i][1] >= 0 ? lut[pl[off[i][1]]] : 0.0f);
      v += wt[i][2] * (off[i][2] >= 0 ? lut[pl[off[i][2]]] : 0.0f);
      v += wt[i][3] * (off[i][3] >= 0 ? lut[pl[off[i][3]]] : 0.0f);
      o[i] = v;
    }
    store_img(img + c * cells, o, n, vec_img);
  }
  if (gt) {
    const unsigned char* __restrict__ expl = snap + plane;
    bool open[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) open[i] = near[i] >= 0 && expl[near[i]] == 0;
    for (int k = 0; k < K; ++k) {
      const unsigned char* __restrict__ tk = last + k * plane;
      unsigned v = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (open[i]) v |= (unsigned)tk[near[i]] << (8 * i);
      store_gt(gt + k * cells, v, n, vec_gt);
    }
  }
}

// scratch of peanut_mapseq_bce: the partials and the [B][K] sums, one buffer per device (the call allocates on the current device,
// as every entry point here launches there).  Under a lock the call holds until its read-back has finished (the call
// synchronises), so no second call can reuse a buffer early.  Never destroyed: no hipFree after the runtime has gone.
std::mutex g_bce_lock;
DevBuf* bce_scratch(int device) {
  static std::map<int, DevBuf*>* per_device = new std::map<int, DevBuf*>();
  DevBuf*& b = (*per_device)[device];
  if (!b) b = new DevBuf();
  return b;
}

int check_seq(const char* who, const peanut_mapseq_t* seq, const peanut_mapseq_sample_t* samples, int B, int S, SampleArgs* P) {
  const std::string w(who);
  if (!seq || !seq->maps || !samples) return fail(PEANUT_EINVAL, w + ": null argument");
  if (seq->T < 1 || seq->C < 1 || seq->W < 1 || seq->H < 1) return fail(PEANUT_EINVAL, w + ": the sequence must be [T,C,W,H] with positive sizes");
  if ((long long)seq->W * seq->H > 0x7fffffffLL) return fail(PEANUT_EINVAL, w + ": a plane of more than 2^31 - 1 cells");
  if (B < 1 || B > PEANUT_MAPSEQ_MAX_SAMPLES) return fail(PEANUT_EINVAL, w + ": B must be 1..PEANUT_MAPSEQ_MAX_SAMPLES");
  if (S < 1 || S > seq->W || S > seq->H) return fail(PEANUT_EINVAL, w + ": the window must be 1..min(W, H)");
  for (int b = 0; b < B; ++b) {
    const peanut_mapseq_sample_t& s = samples[b];
    if (s.t_idx < 0 || s.t_idx >= seq->T) return fail(PEANUT_EINVAL, w + ": t_idx outside [0, T) in sample " + std::to_string(b));
    if (s.x1 < 0 || s.y1 < 0 || s.x1 > seq->W - S || s.y1 > seq->H - S)
      return fail(PEANUT_EINVAL, w + ": the window of sample " + std::to_string(b) + " leaves the map");
    P->t[b] = s.t_idx; P->x1[b] = s.x1; P->y1[b] = s.y1;
  }
  return 0;
}

int grid_for(long long items) {
  const long long blocks = (items + kThreads - 1) / kThreads;
  return (int)std::min<long long>(std::max<long long>(blocks, 1), kMaxBlocks);
}

}  // namespace
}  // namespace peanut

using namespace peanut;

extern "C" {

int peanut_mapseq_encode(const peanut_mapseq_encode_t* batch) {
  if (!batch) return fail(PEANUT_EINVAL, "peanut_mapseq_encode: null argument");
  if (batch->size != sizeof(peanut_mapseq_encode_t)) return fail(PEANUT_EINVAL, "peanut_mapseq_encode: the descriptor's size is not sizeof(peanut_mapseq_encode_t)");
  const int E = batch->E, C = batch->C, W = batch->W, H = batch->H;
  const float* const* src = batch->src;
  const long long *plane_stride = batch->plane_stride, *row_stride = batch->row_stride, *col_stride = batch->col_stride;
  uint8_t* const* dst = batch->dst;
  uint64_t* sums = batch->sums;
  if (E < 1 || E > PEANUT_MAPSEQ_MAX_BATCH) return fail(PEANUT_EINVAL, "peanut_mapseq_encode: E must be 1..PEANUT_MAPSEQ_MAX_BATCH");
  if (!src || !plane_stride || !row_stride || !col_stride || !dst || !sums) return fail(PEANUT_EINVAL, "peanut_mapseq_encode: null argument");
  if (C < 5 || W < 1 || H < 1) return fail(PEANUT_EINVAL, "peanut_mapseq_encode: the map must be [C >= 5, W >= 1, H >= 1]");
  if ((long long)C * W * H > ((long long)1 << 40)) return fail(PEANUT_EINVAL, "peanut_mapseq_encode: map too large");
  EncodeArgs A{};
  for (int e = 0; e < E; ++e) {
    if (!src[e] || !dst[e]) return fail(PEANUT_EINVAL, "peanut_mapseq_encode: null map pointer");
    if (col_stride[e] != 1) return fail(PEANUT_EINVAL, "peanut_mapseq_encode: the column stride must be 1");
    if ((W > 1 && row_stride[e] < H) || plane_stride[e] < 0 || row_stride[e] < 0)
      return fail(PEANUT_EINVAL, "peanut_mapseq_encode: rows overlap (row_stride < H) or a negative stride");
    for (int o = 0; o < e; ++o)
      if (dst[o] == dst[e]) return fail(PEANUT_EINVAL, "peanut_mapseq_encode: two episodes share one dst");
    A.src[e] = src[e]; A.dst[e] = dst[e]; A.plane_stride[e] = plane_stride[e]; A.row_stride[e] = row_stride[e];
    const bool vec = H % 4 == 0 && (uintptr_t)src[e] % 16 == 0 && plane_stride[e] % 4 == 0 && row_stride[e] % 4 == 0 && (uintptr_t)dst[e] % 4 == 0;
    if (vec) A.vec_mask |= 1u << e;
  }
  A.C = C; A.W = W; A.H = H; A.H4 = (H + 3) / 4;
  A.sums = (unsigned long long*)sums;
  hipStream_t s = (hipStream_t)batch->stream;
  PEANUT_HIP_CHECK(hipMemsetAsync(sums, 0, (size_t)E * 2 * sizeof(uint64_t), s));
  mapseq_encode_kernel<<<dim3(grid_for((long long)C * W * A.H4), E), kThreads, 0, s>>>(A);
  PEANUT_HIP_CHECK(hipGetLastError());
  return 0;
}

int peanut_mapseq_inputs(const peanut_mapseq_t* seq, const peanut_mapseq_sample_t* samples, int B, int S, float* out) {
  SampleArgs P{};
  if (int rc = check_seq("peanut_mapseq_inputs", seq, samples, B, S, &P)) return rc;
  if (!out) return fail(PEANUT_EINVAL, "peanut_mapseq_inputs: null argument");
  bool vec = S % 4 == 0 && seq->H % 4 == 0 && (uintptr_t)seq->maps % 4 == 0 && (uintptr_t)out % 16 == 0;
  for (int b = 0; b < B && vec; ++b) vec = P.y1[b] % 4 == 0;
  const int S4 = (S + 3) / 4;
  const dim3 grid(grid_for((long long)seq->C * S * S4), B);
  hipStream_t s = (hipStream_t)seq->stream;
  if (vec) mapseq_inputs_kernel<true><<<grid, kThreads, 0, s>>>(seq->maps, seq->C, seq->W, seq->H, P, S, S4, out);
  else mapseq_inputs_kernel<false><<<grid, kThreads, 0, s>>>(seq->maps, seq->C, seq->W, seq->H, P, S, S4, out);
  PEANUT_HIP_CHECK(hipGetLastError());
  return 0;
}

int peanut_mapseq_bce(const peanut_mapseq_t* seq, const peanut_mapseq_sample_t* samples, int B, int S, const float* logits, int K,
                      double* sum_out) {
  SampleArgs P{};
  if (int rc = check_seq("peanut_mapseq_bce", seq, samples, B, S, &P)) return rc;
  if (!logits || !sum_out) return fail(PEANUT_EINVAL, "peanut_mapseq_bce: null argument");
  if (K < 1 || 4 + K > seq->C) return fail(PEANUT_EINVAL, "peanut_mapseq_bce: K must be 1..C - 4 (the target is channels 4:4 + K)");
  if ((long long)S * S > 0x7fffffffLL - kBceCells) return fail(PEANUT_EINVAL, "peanut_mapseq_bce: window too large");
  const int nchunks = (S * S + kBceCells - 1) / kBceCells;
  const size_t n_part = (size_t)B * K * nchunks, n_sum = (size_t)B * K;
  hipStream_t s = (hipStream_t)seq->stream;
  std::lock_guard<std::mutex> hold(g_bce_lock);
  int device = 0;
  PEANUT_HIP_CHECK(hipGetDevice(&device));
  DevBuf* buf = bce_scratch(device);
  if (int rc = buf->ensure((n_part + n_sum) * sizeof(double))) return rc;
  double* partial = (double*)buf->p;
  double* sum_dev = partial + n_part;
  mapseq_bce_kernel<<<dim3(nchunks, B), kThreads, 0, s>>>(seq->maps, seq->T, seq->C, seq->W, seq->H, P, S, logits, K, partial, nchunks);
  PEANUT_HIP_CHECK(hipGetLastError());
  mapseq_bce_finish_kernel<<<(unsigned)n_sum, kThreads, 0, s>>>(partial, nchunks, sum_dev);
  PEANUT_HIP_CHECK(hipGetLastError());
  PEANUT_HIP_CHECK(hipMemcpyAsync(sum_out, sum_dev, n_sum * sizeof(double), hipMemcpyDeviceToHost, s));
  PEANUT_HIP_CHECK(hipStreamSynchronize(s));
  return 0;
}

int peanut_mapseq_train_batch(const peanut_mapseq_train_t* batch) {
  const std::string w("peanut_mapseq_train_batch");
  if (!batch) return fail(PEANUT_EINVAL, w + ": null argument");
  if (batch->size != sizeof(peanut_mapseq_train_t)) return fail(PEANUT_EINVAL, w + ": the descriptor's size is not sizeof(peanut_mapseq_train_t)");
  const int B = batch->B, C = batch->C, W = batch->W, H = batch->H, K = batch->K;
  const int pad_r = batch->pad_r, pad_c = batch->pad_c, Sr = batch->S_r, Sc = batch->S_c;
  if (!batch->samples || !batch->img) return fail(PEANUT_EINVAL, w + ": null argument");
  if (B < 1 || B > PEANUT_MAPSEQ_MAX_SAMPLES) return fail(PEANUT_EINVAL, w + ": B must be 1..PEANUT_MAPSEQ_MAX_SAMPLES");
  if (C < 5 || W < 1 || H < 1) return fail(PEANUT_EINVAL, w + ": the sequences must be [T, C >= 5, W >= 1, H >= 1]");
  if (K < 1 || K > C - 4) return fail(PEANUT_EINVAL, w + ": K must be 1..C - 4 (the target is channels 4:4 + K)");
  if ((long long)W * H > 0x7fffffffLL) return fail(PEANUT_EINVAL, w + ": a plane of more than 2^31 - 1 cells");
  if (pad_r < W || pad_c < H) return fail(PEANUT_EINVAL, w + ": the pad is smaller than the map");
  if ((long long)pad_r * pad_c > 0x7fffffffLL) return fail(PEANUT_EINVAL, w + ": a padded map of more than 2^31 - 1 cells");
  if (Sr < 1 || Sc < 1 || Sr > pad_r || Sc > pad_c) return fail(PEANUT_EINVAL, w + ": the crop must be 1..pad on both axes");
  const int tiles_r = (Sr + kTileRows - 1) / kTileRows, tiles_c = (Sc + kTileCols - 1) / kTileCols;
  if (tiles_r > 65535) return fail(PEANUT_EINVAL, w + ": crop too tall");
  TrainArgs A{};
  for (int b = 0; b < B; ++b) {
    const peanut_mapseq_aug_t& s = batch->samples[b];
    const std::string at = " in sample " + std::to_string(b);
    if (!s.maps) return fail(PEANUT_EINVAL, w + ": null sequence" + at);
    if (s.T < 1 || s.t_idx < 0 || s.t_idx >= s.T) return fail(PEANUT_EINVAL, w + ": t_idx outside [0, T)" + at);
    if (s.off_r < 0 || s.off_r > pad_r - Sr || s.off_c < 0 || s.off_c > pad_c - Sc)
      return fail(PEANUT_EINVAL, w + ": a crop offset outside [0, pad - S]" + at);
    if (s.flip < 0 || s.flip > 2) return fail(PEANUT_EINVAL, w + ": flip must be 0, 1 or 2" + at);
    if (!std::isfinite(s.cos_t) || !std::isfinite(s.sin_t) || !(std::fabs(s.cos_t * s.cos_t + s.sin_t * s.sin_t - 1.0) <= 1e-9))
      return fail(PEANUT_EINVAL, w + ": (cos_t, sin_t) is not a point of the unit circle" + at);
    TrainSample& d = A.smp[b];
    d.maps = s.maps; d.T = s.T; d.t = s.t_idx; d.oh = s.off_r; d.ow = s.off_c; d.flip = s.flip; d.rotate = s.rotate != 0;
    d.c = s.cos_t; d.s = s.sin_t;
  }
  A.C = C; A.W = W; A.H = H; A.Sr = Sr; A.Sc = Sc; A.K = K;
  A.img = batch->img; A.gt = batch->gt;
  A.vec_img = Sc % 4 == 0 && (uintptr_t)batch->img % 16 == 0;
  A.vec_gt = Sc % 4 == 0 && (uintptr_t)batch->gt % 4 == 0;
  mapseq_train_kernel<<<dim3(tiles_c, tiles_r, B), kThreads, 0, (hipStream_t)batch->stream>>>(A);
  PEANUT_HIP_CHECK(hipGetLastError());
  return 0;
}

int peanut_mapseq_bce_dense(const peanut_mapseq_bce_dense_t* batch) {
  const std::string w("peanut_mapseq_bce_dense");
  if (!batch) return fail(PEANUT_EINVAL, w + ": null argument");
  if (batch->size != sizeof(peanut_mapseq_bce_dense_t)) return fail(PEANUT_EINVAL, w + ": the descriptor's size is not sizeof(peanut_mapseq_bce_dense_t)");
  const int B = batch->B, K = batch->K;
  if (!batch->logits || !batch->gt || !batch->sum_out) return fail(PEANUT_EINVAL, w + ": null argument");
  if (B < 1 || B > PEANUT_MAPSEQ_MAX_SAMPLES) return fail(PEANUT_EINVAL, w + ": B must be 1..PEANUT_MAPSEQ_MAX_SAMPLES");
  if (K < 1 || batch->S_r < 1 || batch->S_c < 1) return fail(PEANUT_EINVAL, w + ": K, S_r and S_c must be positive");
  if ((long long)batch->S_r * batch->S_c > 0x7fffffffLL - kBceCells) return fail(PEANUT_EINVAL, w + ": window too large");
  const int cells = batch->S_r * batch->S_c;
  const int nchunks = (cells + kBceCells - 1) / kBceCells;
  const size_t n_part = (size_t)B * K * nchunks, n_sum = (size_t)B * K;
  hipStream_t s = (hipStream_t)batch->stream;
  std::lock_guard<std::mutex> hold(g_bce_lock);
  int device = 0;
  PEANUT_HIP_CHECK(hipGetDevice(&device));
  DevBuf* buf = bce_scratch(device);
  if (int rc = buf->ensure((n_part + n_sum) * sizeof(double))) return rc;
  double* partial = (double*)buf->p;
  double* sum_dev = partial + n_part;
  mapseq_bce_dense_kernel<<<dim3(nchunks, B), kThreads, 0, s>>>(batch->gt, cells, batch->logits, K, partial, nchunks);
  PEANUT_HIP_CHECK(hipGetLastError());
  mapseq_bce_finish_kernel<<<(unsigned)n_sum, kThreads, 0, s>>>(partial, nchunks, sum_dev);
  PEANUT_HIP_CHECK(hipGetLastError());
  PEANUT_HIP_CHECK(hipMemcpyAsync(batch->sum_out, sum_dev, n_sum * sizeof(double), hipMemcpyDeviceToHost, s));
  PEANUT_HIP_CHECK(hipStreamSynchronize(s));
  return 0;
}

}  // extern "C"
