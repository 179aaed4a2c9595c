// Map datasets on the device (ABI 21): the snapshots nav/collect_maps.py takes of the full map, the model inputs
// prediction/train_prediction_model.py makes of a stored sequence, and the loss it trains with -- all on uint8 sequences that
// stay in device memory.  Three HBM-bound kernels and one small finish kernel; plain HIP, integer atomics only.
#include <algorithm>
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

}  // extern "C"
