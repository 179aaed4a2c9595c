// Stand-alone probe of the persistent A-resident kernel (csrc/conv_pw_ares.hip, included as source): times one pointwise layer and,
// built with -DPEANUT_ARES_TRACE, prints the length of the k-loop iterations of 16 workgroups by kind (first of a unit / steady /
// inside a unit that refills A) from s_memtime stamps -- where an iteration's time goes.  -DPEANUT_ARES_ABL=<bits> removes one cost
// at a time (1: the stores do not execute, 2: no weight requests in the loop, 4: no barrier at the bottom; the result is then
// garbage, only the time means anything); phase 0 removes the half-iteration shift of waves 4-7.  No correctness check here
// (tests/test_conv_gpu.py and tests/test_pw_ares_pipeline_gpu.py hold the kernel to its references).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include -I peanut_amd/csrc [-DPEANUT_ARES_TRACE] [-DPEANUT_ARES_ABL=n] \
//         [-DARES_PROBE_SOURCE='"path/to/another/revision/of/conv_pw_ares.hip"'] tools/micro/ares_probe.hip -o tools/micro/build/ares_probe
//   ares_probe M K N residual(0/1) [reps] [phase(0/1)] [flush(0/1)]          layer3 conv3: 115200 256 1024 1
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#ifndef ARES_PROBE_SOURCE
#define ARES_PROBE_SOURCE "../../peanut_amd/csrc/conv_pw_ares.hip"
#endif
#include ARES_PROBE_SOURCE

namespace peanut {
int fail(int code, const std::string& msg) { fprintf(stderr, "fail %d: %s\n", code, msg.c_str()); return code; }
void note_kernel(const char*) {}
int device_cus() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
  return cus;
}
}  // namespace peanut

__global__ void fill_kernel(float* p, size_t n, unsigned seed, float lo, float scale) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    unsigned h = (unsigned)i * 2654435761u + seed;
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13; h *= 3266489917u; h ^= h >> 16;
    const float u = (float)(h >> 8) * (1.0f / 16777216.0f) * 2.f - 1.f;      // [-1, 1)
    const float v = u * scale;
    p[i] = v < lo ? lo : v;
  }
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main(int argc, char** argv) {
  if (argc < 5) { fprintf(stderr, "usage: ares_probe M K N residual [reps] [phase] [flush]\n"); return 2; }
  const long long M = atoll(argv[1]);
  const int K = atoi(argv[2]), N = atoi(argv[3]), has_res = atoi(argv[4]);
  const int reps = argc > 5 ? atoi(argv[5]) : 20;
  const int phase = argc > 6 ? atoi(argv[6]) : 1;
  const int flush = argc > 7 ? atoi(argv[7]) : 0;
  if (M <= 0 || M % 128 || (K != 128 && K != 256) || N <= 0 || N % 128 || (M / 128) * (N / 128) < 8) { fprintf(stderr, "shape not eligible\n"); return 3; }
  const int abl =
#ifdef PEANUT_ARES_ABL
      PEANUT_ARES_ABL;
#else
      0;
#endif
  float *x, *w, *ss, *res = nullptr, *y, *zeros;
  long long* trace;
  const int kTraceWgs = 16, kTraceLen = 1024;
  CK(hipMalloc(&x, (size_t)M * K * 4));
  CK(hipMalloc(&w, (size_t)N * K * 4));
  CK(hipMalloc(&ss, (size_t)2 * N * 4));
  if (has_res) CK(hipMalloc(&res, (size_t)M * N * 4));
  CK(hipMalloc(&y, (size_t)M * N * 4));
  CK(hipMalloc(&zeros, 4096));
  CK(hipMalloc(&trace, (size_t)kTraceWgs * kTraceLen * 8));
  CK(hipMemset(zeros, 0, 4096));
  CK(hipMemset(trace, 0, (size_t)kTraceWgs * kTraceLen * 8));
  fill_kernel<<<2048, 256>>>(x, (size_t)M * K, 1u, 0.f, 1.7f);            // post-ReLU-like
  fill_kernel<<<2048, 256>>>(w, (size_t)N * K, 3u, -10.f, 1.7f * sqrtf(2.0f / K));
  fill_kernel<<<64, 256>>>(ss, (size_t)N, 4u, 0.5f, 1.5f);
  fill_kernel<<<64, 256>>>(ss + N, (size_t)N, 5u, -1.f, 0.1f);
  if (has_res) fill_kernel<<<2048, 256>>>(res, (size_t)M * N, 6u, -10.f, 1.7f);
  CK(hipDeviceSynchronize());

  peanut::ConvKParams p{};
  p.x = x; p.x2 = x; p.w = w; p.scale = ss; p.shift = ss + N; p.res = res; p.zeros = zeros; p.y = y;
  p.H = 1; p.W = (int)M; p.c1 = K; p.c2 = 0; p.Ho = 1; p.Wo = (int)M; p.cout = N;
  p.kw = 1; p.ntaps = 1; p.stride = 1; p.pad = 0; p.dil = 1; p.relu = 1;
  p.HoWo = (int)M; p.M = (int)M; p.nkt = K / 32; p.ntiles = N / 128;
  p.split_p = 1; p.alpha = 1.f;
  p.flush = flush ? 2 : 0;
  p.partial = reinterpret_cast<float*>(trace);      // the kernel's trace area (PEANUT_ARES_TRACE); the kernel uses no partial tiles
  peanut::Options o = peanut::default_options();
  o.v[peanut::OPT_PW256_PHASE] = phase;
  peanut::OptionScope scope(&o);
  for (int i = 0; i < 3; ++i)
    if (int rc = peanut::launch_conv_pw_ares(p, 128, 0)) { fprintf(stderr, "launch rc %d\n", rc); return 4; }
  CK(hipDeviceSynchronize());
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  CK(hipEventRecord(e0, 0));
  for (int i = 0; i < reps; ++i) peanut::launch_conv_pw_ares(p, 128, 0);
  CK(hipEventRecord(e1, 0));
  CK(hipDeviceSynchronize());
  float ms = 0.f;
  CK(hipEventElapsedTime(&ms, e0, e1));
  ms /= reps;
  printf("{\"M\": %lld, \"K\": %d, \"N\": %d, \"res\": %d, \"phase\": %d, \"flush\": %d, \"abl\": %d, \"ms\": %.4f, \"tflops\": %.1f}\n", M, K, N, has_res, phase,
         flush, abl, ms, 2.0 * M * K * N / ms / 1e9);
#ifdef PEANUT_ARES_TRACE
  {
    // workgroup b < 16 wrote (stamp << 2 | kind) per iteration at [b * 1024 ...], the count at [b * 1024]
    std::vector<long long> tr((size_t)kTraceWgs * kTraceLen);
    CK(hipMemcpy(tr.data(), trace, tr.size() * 8, hipMemcpyDeviceToHost));
    double sum[3] = {0, 0, 0};
    long long cnt[3] = {0, 0, 0};
    double span = 0;
    long long span_n = 0;
    for (int b = 0; b < kTraceWgs; ++b) {
      const long long* t = tr.data() + (size_t)b * kTraceLen;
      const int n = (int)t[0] < kTraceLen - 1 ? (int)t[0] : kTraceLen - 1;
      for (int i = 2; i <= n; ++i) {
        const int kind = (int)(t[i] & 3);
        const long long d = (t[i] >> 2) - (t[i - 1] >> 2);
        if (kind < 3) { sum[kind] += (double)d; cnt[kind]++; }
      }
      if (n >= 2) { span += (double)((t[n] >> 2) - (t[1] >> 2)); span_n += n - 1; }
      if (b == 0) {
        printf("wg0 iterations (kind:ticks): ");
        for (int i = 2; i <= n && i < 80; ++i) printf("%d:%lld ", (int)(t[i] & 3), (t[i] >> 2) - (t[i - 1] >> 2));
        printf("\n");
      }
    }
    // the kernel's whole time is close to the span of a workgroup's stamps: that calibrates a tick
    const double ticks_per_us = span_n ? (span / kTraceWgs) / (ms * 1000.0) : 0;
    printf("{\"trace\": \"mean s_memtime ticks per iteration by kind\", \"first_of_unit\": %.1f, \"steady\": %.1f, \"refill_unit\": %.1f, \"all\": %.1f, "
           "\"n\": [%lld, %lld, %lld], \"ticks_per_us_est\": %.1f}\n",
           cnt[0] ? sum[0] / cnt[0] : 0, cnt[1] ? sum[1] / cnt[1] : 0, cnt[2] ? sum[2] / cnt[2] : 0, span_n ? span / span_n : 0, cnt[0], cnt[1], cnt[2],
           ticks_per_us);
  }
#endif
  return 0;
}
