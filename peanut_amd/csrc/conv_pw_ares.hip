// Short-K pointwise convs and Winograd position GEMMs (K = 128 or 256 input channels) as a PERSISTENT, A-RESIDENT kernel.
//
// Why: the expanding 1x1 convs of a Bottleneck (resnet.py:267-307 conv3: K = C/4 -> N = C, + identity, ReLU) and the
// position GEMMs of the narrow Winograd layers are 4-8 k-tiles long.  On the tile-per-workgroup kernels of conv_pw.hip
// every 128 x 64 tile pays a pipeline fill, an epilogue with nothing under it and a workgroup launch per 6.8 us of
// matrix-core work: the family runs at 96 TF/s with the matrix pipes busy 0.635 of the cycles (profiles/r4o), and a
// layer's time is its MFMA time PLUS its HBM time.
//
// Here one workgroup per CU (8 waves, wave tile 64 x 32) walks a contiguous range of (m-tile, n-tile) units, n fastest:
//   * the 128 x K A tile of the current m-tile stays in LDS (K / 32 slices of 16 KiB) while the n-tiles pass by; when
//     the last n-tile of an m-tile has read a slice for the last time, that slice is refilled IN PLACE with the next
//     m-tile's, so the A stream never stops either;
//   * only the weights stream: one 128 x 32 k-tile (16 KiB) per iteration into a two-stage ring, requested a full
//     iteration ahead, across unit boundaries -- no per-tile prologue;
//   * the epilogue of unit u runs INSIDE the k-loop of unit u + 1, from registers: the finished accumulators are copied
//     to a second register set, and every iteration finishes 32 / (K/32) of them per lane -- residual loads at the top
//     of the iteration (hidden from hipcc's wait-count bookkeeping: inline asm, cdna_hip_programming.md 5.7 form (ii)),
//     scale / shift / add / ReLU after the MFMAs into a few HELD registers, their stores behind the next iteration's
//     weight request (protocol below).  A lane's 32 values are rows x one column, a wave instruction covers two rows x 32
//     consecutive channels = two whole 128-byte lines;
//   * the two waves of a SIMD request their LDS-DMA pieces half an iteration apart (see conv_pw_glds256_kernel).
// Arithmetic: the same MFMA fragment layout and k order as the other fp32 kernels, so results are bit-identical to theirs
// (two-level accumulation every 64 channels included: FLUSH).
//
// LDS: (K/32 + 2) x 16 KiB = all 160 KiB at K = 256.
//
// vmcnt protocol per iteration and wave (loads and stores of one wave retire in issue order, which hipcc's own counted
// waits rely on as well).  Issue order inside iteration t:
//   1. the residual loads of chunk t (asm, not counted by hipcc), at the top;
//   2. the two A refill pieces of the slice iteration t - 1 read last, at the top (refill units only; that slice is free
//      since the barrier that ended t - 1);
//   3. the two weight pieces of k-tile t + 1 (LDS-DMA), at the top or -- waves 4-7, option pw256_phase -- after 16 MFMAs;
//   4. right behind them the CH stores of chunk t - 1, whose finished values were HELD in registers over the last barrier.
// The bottom wait is `s_waitcnt vmcnt(CH)`: it retires 1-3 and leaves exactly the CH stores of 4 in flight, so a store has
// until the bottom wait of iteration t + 1 -- two iterations from the moment its value was finished -- to be acknowledged,
// instead of one.  After the wait chunk t is finished into the held registers, and the barrier publishes the landed pieces.
// The number of operations behind the weight request is a compile-time constant of the iteration: the first unit of a
// range (no previous unit) and k-tile 0 of its second unit (nothing held yet) are separate instantiations of the unit body
// that issue no stores and wait `vmcnt(0)`.  The drain issues the held chunk, finishes the last unit's chunks with nothing
// under them and ends in `vmcnt(0)`.
// A refill: slice kt - 1 of the next m-tile is requested at the top of iteration kt of the m-tile's last unit (slice NK - 1 at
// the top of the next unit's k-tile 0), retired by that iteration's bottom wait and published by its barrier; it is first
// read NK - 1 iterations after the one that read it last.
// Measured stand-alone (tools/micro/ares_probe.hip, profiles/r10a): with the stores issued right after the wait and every wait
// a `vmcnt(0)` the stores cost 12 % of a steady iteration (layer3 conv3's shape, 103-104.5 TF/s); held for one iteration they
// cost under 3 % (108.5-109.8 TF/s; 86-87 -> 92-92.6 on a position GEMM with K = N = 256, 86 -> 90 at K = 128).  What is
// left of the gap to the matrix pipe is the weight request (3 %), the barrier (7 %) and the fragment reads at the top.
#include <stdlib.h>

#include "common.h"
#include "conv_common.h"

namespace peanut {

namespace {

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

// A global load hipcc does not count (cdna_hip_programming.md 5.7, form (iii)): the destination is valid only after the
// caller's wait_uncounted(); every such load is unconditional and its result is read only below that wait, so that no
// compiler copy of a destination can sit between the load and the wait (tests/test_abi.py audits the generated code).
// Wave-uniform base in SGPRs + a 32-bit lane offset in bytes.  The leading s_nop covers the case that hipcc materialised the base
// through v_readfirstlane right before the statement (VALU-written SGPR read by a VMEM instruction: 5 wait states hipcc does
// not pad inside an asm).
__device__ __forceinline__ float load_uncounted(const float* base, unsigned byte_off) {
  float v;
  asm volatile("s_nop 4\n\tglobal_load_dword %0, %1, %2" : "=v"(v) : "v"(byte_off), "s"(base) : "memory");
  return v;
}
// The wait names every destination as an INPUT: that keeps the registers allocated to the loads until the data has landed
// even on paths where the values are not used afterwards (first unit, no previous epilogue) -- hipcc would otherwise hand a
// dead destination to something else while its load is still in flight.
// N: the youngest vector-memory operations of the wave that may stay in flight (the held chunk's stores, or none).
template <int CH, int N>
__device__ __forceinline__ void wait_uncounted(const float (&r)[CH], float a, float b) {
  static_assert(CH == 4 || CH == 8, "chunk of 4 or 8 values");
  static_assert(N == 0 || N == CH, "nothing, or the stores of one chunk");
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (CH == 4)
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N), "v"(r[0]), "v"(r[1]), "v"(r[2]), "v"(r[3]), "v"(a), "v"(b) : "memory");
  else
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N), "v"(r[0]), "v"(r[1]), "v"(r[2]), "v"(r[3]), "v"(r[4]), "v"(r[5]), "v"(r[6]), "v"(r[7]), "v"(a),
                 "v"(b)
                 : "memory");
  __builtin_amdgcn_sched_barrier(0);
}

template <int NK, bool FLUSH>
__global__ __launch_bounds__(512) void conv_pw_ares_kernel(const ConvKParams p) {
  constexpr int BK = 32, K = NK * BK, TILE = 128 * BK;   // TILE: floats of one 128-row k-tile (16 KiB)
  constexpr int CH = 32 / NK;                            // accumulator registers of the previous unit finished per iteration
  static_assert(NK == 4 || NK == 8, "K = 128 or 256");
  __shared__ __attribute__((aligned(1024))) float smem[(NK + 2) * TILE];
  float* const bst = smem + NK * TILE;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane >> 3, lp = lane & 7;
  const int wm = wave >> 2, wn = wave & 3;               // 2 x 4 waves, wave tile 64 x 32
  const int li = lane & 31, hi = lane >> 5;
  const bool late = p.phase_shift && wave >= 4;

  // ---- this workgroup's units: a contiguous range of (m-tile, n-tile), n fastest; neighbouring ranges on one XCD ----
  const int G = gridDim.x, bid = blockIdx.x;
  const int lw = (bid & 7) * (G >> 3) + (bid >> 3);      // the launcher keeps G a multiple of 8
  const int NT = p.ntiles;
  const long long U = (long long)p.mtiles * NT;
  const int u0 = (int)(U * lw / G), u1 = (int)(U * (lw + 1) / G);
  if (u0 >= u1) return;

  // ---- lane constants of the LDS-DMA pieces: two 8-row pieces of A and of B per wave and k-tile ----
  const int pbn = p.ares_pbn;                            // n-tile the weights were packed with (64 or 128)
  unsigned a_off[2], b_off[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int r = (wave * 2 + j) * 8 + lr;
    const int c = lp ^ ((r >> 1) & 7);
    a_off[j] = r * K + c * 4;
    b_off[j] = (r / pbn) * (NK * pbn * BK) + (r % pbn) * BK + c * 4;
  }
  auto dma_a = [&](int mt, int s) {     // slice s of m-tile mt -> smem[s]
    const float* base = p.x + (size_t)mt * (128 * K) + s * BK;
#pragma unroll
    for (int j = 0; j < 2; ++j)
      __builtin_amdgcn_global_load_lds((gptr_t)(base + a_off[j]), (lptr_t)(smem + s * TILE + (wave * 2 + j) * 256), 16, 0, 0);
  };
  auto dma_b = [&](int mt, int nt, int kt, int stage) {
    const float* base = p.w + (p.mt_per_group ? (size_t)(mt / p.mt_per_group) * p.w_group_stride : 0) + (size_t)nt * (128 * K) + kt * (pbn * BK);
#pragma unroll
    for (int j = 0; j < 2; ++j)
      __builtin_amdgcn_global_load_lds((gptr_t)(base + b_off[j]), (lptr_t)(bst + stage * TILE + (wave * 2 + j) * 256), 16, 0, 0);
  };

  // ---- MFMA fragment coordinates (conv_pw.hip's swizzle) ----
  const int swz = (li >> 1) & 7;
  int sw[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) sw[ks] = ((ks * 2 + hi) ^ swz) * 4;
  const int a_row = (wm * 64 + li) * BK;
  const int b_row = (wn * 32 + li) * BK;

  f32x16 acc[2], acc2[2], prev[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[t][r] = 0.f; acc2[t][r] = 0.f; prev[t][r] = 0.f; }

  // ---- epilogue addressing.  Lane (wm, wn, li, hi) holds column wn*32 + li of rows wm*64 + 4*hi + rowoff(idx), idx = 0..31 the
  // linear index into its two f32x16, rowoff(idx) = 8 * (idx >> 2) + (idx & 3): four consecutive rows, then a jump of eight.
  // Residual and output are walked by running per-lane pointers.  Without a residual the loads read the zero page (stride 0).
  const unsigned lane_el = (unsigned)(wm * 64 + 4 * hi) * p.cout + wn * 32 + li;      // inside one 128-row tile: 32 bits
  const bool has_res = p.res != nullptr;
  // A unit's tile is a wave-uniform base (SGPRs); inside it a lane walks 32-bit byte offsets (a tile spans 128 * cout * 4 bytes).
  const unsigned rstride = has_res ? (unsigned)p.cout * 4u : 0u;
  const unsigned ostride = (unsigned)p.cout * 4u;
  const float* res_base = has_res ? p.res : p.zeros;     // previous unit's residual tile ...
  unsigned res_off = has_res ? lane_el * 4u : 0u;        // ... advanced chunk by chunk as it is loaded
  float* out_base = p.y;                                 // the tile of the chunk that is stored next ...
  unsigned out_off = lane_el * 4u;                       // ... advanced chunk by chunk as it is STORED
  const unsigned ss_lane = (unsigned)(wn * 32 + li) * 4u;
  float scv = 1.f, shv = 0.f;
  const float alpha = p.alpha;
  const bool relu = p.relu != 0;
  float held[CH];                        // the chunk finished last: stored behind the NEXT iteration's weight request
  // unit u's tile in residual / output, and its columns in scale / shift (worked out when its epilogue opens, not carried)
  auto unit_el = [&](int u) {
    const int mt = u / NT, nt = u - mt * NT;
    return (size_t)mt * 128 * p.cout + (size_t)nt * 128;
  };
  auto unit_ss = [&](int u) {
    const int mt = u / NT, nt = u - mt * NT;
    const int ss_off = (p.mt_per_group && p.ss_group_stride) ? (mt / p.mt_per_group) * p.ss_group_stride : 0;
    return ss_off + nt * 128;
  };

  // one chunk of the previous unit's epilogue, split around the MFMAs: loads at the top, the values after wait_uncounted(),
  // their stores one iteration later
#define ARES_CHUNK_LOADS(kt, ss)                                                          \
  float resv[CH];                                                                         \
  if ((kt) == 0) {                                                                        \
    scv = load_uncounted(p.scale + (ss), ss_lane);                                        \
    shv = load_uncounted(p.shift + (ss), ss_lane);                                        \
  }                                                                                       \
  _Pragma("unroll") for (int i = 0; i < CH; ++i)                                          \
    resv[i] = load_uncounted(res_base, res_off + (unsigned)(8 * (i >> 2) + (i & 3)) * rstride); \
  res_off += (unsigned)(2 * CH) * rstride;
#define ARES_CHUNK_FINISH(kt)                                                             \
  _Pragma("unroll") for (int i = 0; i < CH; ++i) {                                        \
    const int idx = (kt) * CH + i;                                                        \
    float v = prev[idx >> 4][idx & 15] * (scv * alpha) + shv;                             \
    v += resv[i];                                                                         \
    if (relu) v = relu_keep_nan(v);                                                       \
    held[i] = v;                                                                          \
  }
#define ARES_STORE_HELD()                                                                 \
  _Pragma("unroll") for (int i = 0; i < CH; ++i)                                          \
    *reinterpret_cast<float*>(reinterpret_cast<char*>(out_base) + (out_off + (unsigned)(8 * (i >> 2) + (i & 3)) * ostride)) = held[i]; \
  out_off += (unsigned)(2 * CH) * ostride;

  // ---- prologue: the whole A tile of the first m-tile and the first weight k-tile ----
  {
    const int mt = u0 / NT, nt = u0 - mt * NT;
#pragma unroll
    for (int s = 0; s < NK; ++s) dma_a(mt, s);
    dma_b(mt, nt, 0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  }

#ifdef PEANUT_ARES_TRACE     // tools/micro/ares_probe.hip: s_memtime stamp of every iteration's end, by kind, for the first 16 workgroups
  long long* const trace = reinterpret_cast<long long*>(p.partial) + blockIdx.x * 1024;
  int trace_n = 0;
#define ARES_TRACE(kind)                                                                                      \
  if (blockIdx.x < 16 && tid == 0) {                                                                          \
    ++trace_n;                                                                                                \
    if (trace_n < 1024) trace[trace_n] = (long long)(__builtin_amdgcn_s_memtime() << 2) | (kind);             \
    trace[0] = trace_n;                                                                                       \
  }
#else
#define ARES_TRACE(kind)
#endif
#ifndef PEANUT_ARES_ABL      // the probe's ablations (never set in the library): 1 the stores do not execute, 2 no weight requests
#define PEANUT_ARES_ABL 0    // in the loop (a stage that never changes), 4 no barrier at the bottom.  Results are then garbage.
#endif

  int stage = 0;
  // One unit.  V: 0 = the first unit of the range (no previous unit, so no epilogue under it), 1 = the second (nothing is held
  // yet at its k-tile 0), 2 = every later one.  V fixes how many stores follow each weight request, hence each wait's count.
  auto run_unit = [&](const int u, auto vc) {
    constexpr int V = decltype(vc)::value;
    const int mt = u / NT, nt = u - mt * NT;
    const bool nxt = u + 1 < u1;
    const int mt_n = nxt ? (u + 1) / NT : mt;
    const int nt_n = nxt ? (u + 1) - mt_n * NT : 0;
    const bool refill_next = nxt && mt_n != mt;     // this unit is the last reader of its m-tile's slices: refill them for the next
    const bool refill_last = V > 0 && (u - 1) / NT != mt;   // ... and the previous unit was: its last slice is free only now
    const int ss = unit_ss(V > 0 ? u - 1 : u);
    if (V > 0) {
      if (has_res) res_base = p.res + unit_el(u - 1);
      res_off = has_res ? lane_el * 4u : 0u;
    }
    // opaque: the offsets restart at the same value in every unit, and hipcc would keep all 32 rows' offsets of both walks in
    // registers across the unit loop
    asm volatile("" : "+v"(res_off));

    static_for<NK>([&](auto kc) {
      constexpr int kt = decltype(kc)::value;
      constexpr bool STORES = !(PEANUT_ARES_ABL & 1) && (V == 2 || (V == 1 && kt >= 1));
      const float* const cur_b = bst + stage * TILE;
      const float* const cur_a = smem + kt * TILE;
      const bool more = !(PEANUT_ARES_ABL & 2) && ((kt + 1 < NK) || nxt);
      // -- top: residual loads of this iteration's chunk of the previous unit; the refill of the slice the previous iteration
      // read last; the next weight k-tile and, behind it, the stores of the chunk held since the previous iteration --
      ARES_CHUNK_LOADS(kt, ss)
      if (kt >= 1) { if (refill_next) dma_a(mt_n, kt - 1); }
      else { if (refill_last) dma_a(mt, NK - 1); }
      auto request = [&]() {
        if (more) {
          if (kt + 1 < NK) dma_b(mt, nt, kt + 1, stage ^ 1);
          else dma_b(mt_n, nt_n, 0, stage ^ 1);
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (STORES) { ARES_STORE_HELD() }
        else if constexpr ((PEANUT_ARES_ABL & 1) != 0) { if (p.pad) { ARES_STORE_HELD() } }
        if constexpr (V > 0 && kt == 0) {      // the held chunk was the last of the unit before
          out_base = p.y + unit_el(u - 1);
          out_off = lane_el * 4u;
          asm volatile("" : "+v"(out_off));
        }
      };
      if (!late) request();
      __builtin_amdgcn_sched_barrier(0);
      // -- 32 MFMAs: four 8-k groups of (2 A fragments, 1 B fragment) --
      f32x4 af[4][2], bf[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        af[j][0] = *reinterpret_cast<const f32x4*>(cur_a + a_row + sw[j]);
        af[j][1] = *reinterpret_cast<const f32x4*>(cur_a + a_row + 32 * BK + sw[j]);
        bf[j] = *reinterpret_cast<const f32x4*>(cur_b + b_row + sw[j]);
      }
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
          for (int t = 0; t < 2; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[j][t][kk], bf[j][kk], acc[t], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      if (late) request();
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 2; j < 4; ++j)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
#pragma unroll
          for (int t = 0; t < 2; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[j][t][kk], bf[j][kk], acc[t], 0, 0, 0);
      if (FLUSH && (kt & 1)) {      // partial sums of 64 channels (conv_common.h: PEANUT_FLUSH_*)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          acc2[t] += acc[t];
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
        }
      }
      // -- bottom: everything this wave has requested has landed, but for the stores behind the weight request; finish the
      // chunk into the held registers --
      wait_uncounted<CH, STORES ? CH : 0>(resv, scv, shv);
      ARES_TRACE(kt == 0 ? 0 : (refill_next ? 2 : 1))
      if constexpr (V > 0) { ARES_CHUNK_FINISH(kt) }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if constexpr (!(PEANUT_ARES_ABL & 4)) __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      stage ^= 1;
    });

    // unit finished: its accumulators become the "previous" set, the epilogue pointers move to its tile
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      prev[t] = FLUSH ? acc2[t] : acc[t];
#pragma unroll
      for (int r = 0; r < 16; ++r) { acc[t][r] = 0.f; acc2[t][r] = 0.f; }
    }
  };
  {
    int u = u0;
    run_unit(u++, IC<0>{});
    if (u < u1) run_unit(u++, IC<1>{});
    for (; u < u1; ++u) run_unit(u, IC<2>{});
  }

  // ---- drain: the chunk still held (ranges of two units or more), then the last unit's epilogue with nothing under it ----
  if (!(PEANUT_ARES_ABL & 1) || p.pad) {
    if (u1 - u0 >= 2) { ARES_STORE_HELD() }
    out_base = p.y + unit_el(u1 - 1);
    out_off = lane_el * 4u;
    if (has_res) res_base = p.res + unit_el(u1 - 1);
    res_off = has_res ? lane_el * 4u : 0u;
    const int ss = unit_ss(u1 - 1);
    static_for<NK>([&](auto kc) {
      constexpr int kt = decltype(kc)::value;
      ARES_CHUNK_LOADS(kt, ss)
      wait_uncounted<CH, 0>(resv, scv, shv);
      ARES_CHUNK_FINISH(kt)
      ARES_STORE_HELD()
    });
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#undef ARES_CHUNK_LOADS
#undef ARES_CHUNK_FINISH
#undef ARES_STORE_HELD
#undef ARES_TRACE
}

template <int NK, bool FLUSH>
int launch_ares_t(ConvKParams p, hipStream_t stream) {
  const int cus = device_cus();
  if (cus < 8) return fail(-3, "conv_pw_ares: no current device");
  const long long U = (long long)p.mtiles * p.ntiles;
  long long G = U < cus ? U : cus;
  G -= G % 8;
  if (G < 8) return fail(-2, "conv_pw_ares: launch too small");
  hipLaunchKernelGGL((conv_pw_ares_kernel<NK, FLUSH>), dim3((unsigned)G), dim3(512), 0, stream, p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(-3, std::string("conv_pw_ares launch: ") + hipGetErrorString(e));
  return 0;
}

}  // namespace

// Which pointwise layers / grouped GEMMs take the A-resident kernel: K = 128 or 256 from one source, stride 1, whole
// 128-row and 128-column tiles (every Bottleneck conv3 and Winograd position GEMM of the prediction net at batch sizes
// that fill the chip), one running sum or partial sums of 64 channels, and at least pw_ares_minunits units (two
// per CU).  Option pw_ares = 0 switches the kernel off (options.h).
bool conv_pw_uses_ares(int cin, int cout, long long M, int stride, bool two_source, int flush_ktiles, int bn_tile) {
  const bool on = opt(OPT_PW_ARES) != 0;
  const long long min_units = opt(OPT_PW_ARES_MINUNITS);
  if (!on || two_source || (cin != 128 && cin != 256) || stride != 1 || M % 128 != 0 || cout % 128 != 0) return false;
  if (bn_tile != 64 && bn_tile != 128) return false;
  if (flush_ktiles != 0 && flush_ktiles != 2) return false;
  return (M / 128) * (cout / 128) >= min_units;
}

int launch_conv_pw_ares(const ConvKParams& p0, int bn_tile, hipStream_t stream) {
  ConvKParams p = p0;
  p.phase_shift = opt(OPT_PW256_PHASE) != 0;
  p.ares_pbn = bn_tile;
  p.mtiles = p.M / 128;
  p.ntiles = p.cout / 128;
  const bool flush = p.flush == 2;
  if (p.c1 == 256) return flush ? launch_ares_t<8, true>(p, stream) : launch_ares_t<8, false>(p, stream);
  return flush ? launch_ares_t<4, true>(p, stream) : launch_ares_t<4, false>(p, stream);
}

}  // namespace peanut
