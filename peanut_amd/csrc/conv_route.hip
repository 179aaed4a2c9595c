// Which kernel runs a conv layer: ONE pure host function, asked by the launcher (launch_conv, below) and by the planners'
// op tables (pred_api.hip, rcnn_api.hip) alike, and the one table of kernel family names ("The conv route").
#include "common.h"
#include "conv_common.h"
#include "rs_common.h"

namespace peanut {

// CUs of the current device: one query per device (0: no current device)
int device_cus() {
  static std::atomic<int> cached[SlotCache::kMaxDevices];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return 0;
  const bool in_cache = dev < SlotCache::kMaxDevices;      // (a higher ordinal is asked every time)
  int cus = in_cache ? cached[dev].load(std::memory_order_relaxed) : 0;
  if (cus == 0) {
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    if (in_cache) cached[dev].store(cus, std::memory_order_relaxed);
  }
  return cus;
}

namespace {

ConvRoute route_of(ConvKernelId id, int bm = 0, int bn = 0, int bk = 0) {
  ConvRoute r{};
  r.id = id; r.bm = bm; r.bn = bn; r.bk = bk;
  return r;
}
ConvRoute no_route(int code, const char* why) {
  ConvRoute r{};
  r.id = CONV_K_INVALID; r.code = code; r.error = why;
  return r;
}

// fp32, BK = 32, 1x1, pad 0, sources of whole k-tiles (checked by conv_route)
ConvRoute route_pw(const ConvKParams& p, int bn_tile, size_t ws_floats) {
  // a handful of data rows per weight group (the PSP pyramid at batch 1): weight streaming, no LDS (gemm_skinny.hip)
  if (gemm_skinny_takes(p, bn_tile, ws_floats)) return route_of(CONV_K_GEMM_SKINNY);
  const bool streamk = opt(OPT_PW256P_STREAMK) != 0;
  // (the persistent 256 x 256 kernel first: its gate starts at 512 input channels by default, above the A-resident kernel's K = 128 / 256
  // layers; lowering pw256wp_mink hands those to it)
  if (conv_pw_uses_256wp(p.cout, p.M, p.stride, p.mt_per_group, bn_tile, p.c1, p.c2, p.flush)) {
    const int cus = device_cus();
    if (cus < 8) return no_route(-3, "conv_pw256wp: no current device");
    ConvRoute r = route_of(CONV_K_PW_256X256P, 256, 256, 32);
    r.G = cus - cus % 8;          // one workgroup per CU whatever the tile count: a launch with fewer tiles than CUs is all split parts
    r.plan = plan_persistent((p.M / 256) * (p.cout / 256), r.G, p.nkt, kPersistent256x256, streamk, ws_floats);
    if (r.plan.fits) return r;    // else (no room for the partial tiles + the dump tile, or for the items): the kernels below
  }
  if (conv_pw_uses_ares(p.c1, p.cout, p.M, p.stride, p.c2 != 0, p.flush, bn_tile)) return route_of(CONV_K_PW_ARES, 128, 128, 32);
  if (conv_pw_uses_256w(p.cout, p.M, p.mt_per_group, bn_tile, p.c1 + p.c2, p.flush)) return route_of(CONV_K_PW_256X256, 256, 256, 32);
  if (conv_pw_uses_256p(p.cout, p.M, p.mt_per_group, bn_tile, p.c1 + p.c2, p.flush, (long long)(p.M / p.HoWo) * p.H * p.W) && !(p.flush && p.res)) {
    const int cus = device_cus();
    if (cus < 8) return no_route(-3, "conv_pw256p: no current device");
    ConvRoute r = route_of(CONV_K_PW_256X128P, 256, 128, 32);
    r.G = cus - cus % 8;
    r.plan = plan_persistent(((p.M + 255) / 256) * p.ntiles, r.G, p.nkt, p.flush ? kPersistent256x128Flush : kPersistent256x128, streamk, ws_floats);
    // (a uniform split whose parts do not fit the scratch stays this kernel's launch, which fails; more items per workgroup than the
    // plan table holds -- a layer near the 4 GiB output bound, or a part with few CUs -- goes to the tile-per-workgroup kernels)
    if (r.plan.fits || !r.plan.scratch_ok) return r;
  }
  if (conv_pw_uses_256(p.cout, p.M, p.mt_per_group, bn_tile, p.c1 + p.c2)) return route_of(CONV_K_PW_256X128, 256, 128, 32);
  if (conv_pw_narrow_tiles(p.c1 + p.c2, p.cout, p.M, bn_tile, p.mt_per_group)) {      // 64-wide tiles over 128-wide packing
    ConvRoute r = route_of(CONV_K_PW_TILE, 128, 64, 32);
    r.pack_bn = 128;
    return r;
  }
  if (bn_tile != 128 && bn_tile != 64 && bn_tile != 32) return no_route(-2, "launch_conv_pw: unsupported tile configuration");
  return route_of(CONV_K_PW_TILE, 128, bn_tile, 32);
}

}  // namespace

ConvRoute conv_route(const ConvDesc& d, const ConvArgs& a, ConvKParams* params) {
  if (a.c1 + a.c2 != d.cin) return no_route(-2, "launch_conv: c1 + c2 != cin");
  // gemm_rs.hip reads two sources at one pixel stride only for stride 1; a strided two-source pointwise layer of an emulated
  // mode runs on the fp32 MFMA kernels instead (its fp32-packed weights are always uploaded; exact fp32: nothing is lost)
  const bool rs_fallback = d.rs == 1 && a.c2 != 0 && d.stride != 1;
  const bool emulated = d.rs && !rs_fallback;
  const int kgran = emulated ? 16 : d.bk;     // k-tile of the kernel that will run
  if (a.c1 % kgran != 0 || (a.c2 % kgran) != 0) return no_route(-2, "launch_conv: channel split not a multiple of the k-tile");
  ConvKParams local;
  ConvKParams& p = params ? *params : local;
  p = ConvKParams{};
  p.x = a.x; p.x2 = a.x2 ? a.x2 : a.x; p.w = d.w_packed; p.scale = d.scale; p.shift = d.shift;
  p.res = a.res; p.y = a.y;
  p.H = a.H; p.W = a.W; p.c1 = a.c1; p.c2 = a.c2; p.Ho = a.Ho; p.Wo = a.Wo; p.cout = d.cout;
  p.kw = d.kw; p.ntaps = d.kh * d.kw; p.stride = d.stride; p.pad = d.pad; p.dil = d.dil; p.relu = d.relu;
  p.HoWo = a.Ho * a.Wo;
  const long long M = (long long)a.B * p.HoWo;
  if (M <= 0 || M > 0x7fffffffLL || (long long)a.B * a.H * a.W > 0x7fffffffLL)
    return no_route(-2, "launch_conv: problem size out of range");
  p.M = (int)M;
  p.nkt = (d.cin / d.bk) * p.ntaps;
  p.ntiles = d.cout_pad / d.bn_tile;
  p.n_full = 0; p.n_sp = 0; p.split_p = 1; p.partial = nullptr;
  p.alpha = 1.f;
  p.flush = emulated ? 0 : d.flush_ch / d.bk;   // k-tiles per partial sum (conv_pw.hip; every other kernel keeps one running sum)
  p.mt_per_group = a.mt_per_group; p.w_group_stride = (long long)a.w_group_stride; p.ss_group_stride = a.ss_group_stride;
  p.group_valid = a.mt_per_group ? a.group_valid_rows : 0;
  p.defer = a.defer;
  p.group_rows = a.mt_per_group ? a.group_rows : nullptr;
  if (emulated) {   // emulated-fp32 GEMM on the bf16 matrix cores, fp32 activations split in registers
    p.w = static_cast<const float*>(d.w_s);
    p.nkt = (d.cin / 16) * p.ntaps;
    p.alpha = d.s_alpha;
    ConvRoute r = route_of(CONV_K_CONV_RS, 128, d.bn_tile, 16);
    if (d.rs != 2) {
      const int cin = p.c1 + p.c2;
      if (gemm_rs_uses_64(p.cout, p.M, d.bn_tile, cin)) r = route_of(CONV_K_GEMM_RS, 64, 64, 16);
      else if (gemm_rs_uses_256(p.cout, p.M, p.mt_per_group, d.bn_tile, cin)) r = route_of(CONV_K_GEMM_RS, 256, 256, 16);
      else r = route_of(CONV_K_GEMM_RS, 128, d.bn_tile == 128 ? 128 : 64, 16);
    }
    r.planes = d.s_planes;
    return r;
  }
  if (d.bk == 32 && p.ntaps == 1 && p.pad == 0 && p.c1 % 32 == 0 && p.c2 % 32 == 0 && (p.c2 == 0 || p.stride == 1) && conv_pw_enabled())
    return route_pw(p, d.bn_tile, a.ws ? a.ws_floats : 0);
  if (conv_patch_eligible(d, a)) {
    ConvRoute r = route_of(CONV_K_PATCH, 0, d.cout, d.cin);      // (a patch layer is packed with bk = cin)
    r.stride = d.stride;
    return r;
  }
  if ((d.bk != 32 && d.bk != 16) || (d.bn_tile != 128 && d.bn_tile != 64 && d.bn_tile != 32))
    return no_route(-2, "launch_conv: unsupported tile configuration");
  return route_of(CONV_K_IGEMM, 128, d.bn_tile, d.bk);
}

// build the launch parameters, choose the kernel, run it
int launch_conv(const ConvDesc& d, const ConvArgs& a, hipStream_t stream) {
  ConvKParams p;
  const ConvRoute r = conv_route(d, a, &p);
  if (r.id == CONV_K_INVALID) return fail(r.code, r.error);
  p.zeros = zero_page();
  if (!p.zeros) return fail(-3, "launch_conv: zero page allocation failed");
  if (a.defer) a.defer->valid = false;      // set by launch_with_tail_split alone, when it left its partial tiles unsummed
  if ((r.id == CONV_K_GEMM_RS || r.id == CONV_K_CONV_RS) && !d.w_s) return fail(-2, "launch_conv: register-split layer without pre-split weights");
  note_kernel(conv_kernel_family(r));
  switch (r.id) {
    case CONV_K_GEMM_RS: return launch_gemm_rs(p, r, d.bn_tile, a.ws, a.ws_floats, stream);
    case CONV_K_CONV_RS: return launch_conv_rs(p, d.bn_tile, d.s_planes, a.ws, a.ws_floats, stream);
    case CONV_K_GEMM_SKINNY: return launch_gemm_skinny(p, a.ws, a.ws_floats, stream);
    case CONV_K_PW_256X256P: return launch_conv_pw256wp(p, r, a.ws, stream);
    case CONV_K_PW_ARES: return launch_conv_pw_ares(p, d.bn_tile, stream);
    case CONV_K_PW_256X128P: return launch_conv_pw256p(p, r, a.ws, stream);
    case CONV_K_PW_256X256:
    case CONV_K_PW_256X128:
    case CONV_K_PW_TILE: return launch_conv_pw(p, r, a.ws, a.ws_floats, stream);
    case CONV_K_PATCH: return launch_conv_patch(p, d, a.B, stream);
    case CONV_K_IGEMM: return launch_conv_igemm(p, d.bn_tile, d.bk, a.ws, a.ws_floats, stream);
    case CONV_K_PATCH_NCHW:
    case CONV_K_INVALID: break;
  }
  return fail(-2, "launch_conv: no kernel");
}

ConvRoute conv_route_patch_nchw() {
  ConvRoute r = route_of(CONV_K_PATCH_NCHW, 0, 32, 16);
  r.stride = 2;
  return r;
}

// THE name table: the family string of every conv kernel (peanut_last_conv_kernel, the planners' op tables, bench.py's attribution)
const char* conv_kernel_family(const ConvRoute& r) {
  const int ni = r.bn == 128 ? 0 : (r.bn == 64 ? 1 : 2);              // 128 / 64 / 32 columns
  const int kind = r.planes - RS_BF16X3;                               // emulation kinds: bf16x3, bf16x6, fp16x3
  switch (r.id) {
    case CONV_K_INVALID: break;
    case CONV_K_IGEMM: {
      static const char* const names[2][3] = {{"conv_igemm_128x128x32", "conv_igemm_128x64x32", "conv_igemm_128x32x32"},
                                              {"conv_igemm_128x128x16", "conv_igemm_128x64x16", "conv_igemm_128x32x16"}};
      return names[r.bk == 32 ? 0 : 1][ni];
    }
    case CONV_K_CONV_RS: {
      static const char* const names[3][3] = {{"conv_rs3_128x128", "conv_rs3_128x64", "conv_rs3_128x32"},
                                              {"conv_rs6_128x128", "conv_rs6_128x64", "conv_rs6_128x32"},
                                              {"conv_rs3h_128x128", "conv_rs3h_128x64", "conv_rs3h_128x32"}};
      return kind < 0 || kind > 2 ? "conv_rs?" : names[kind][ni];
    }
    case CONV_K_GEMM_RS: {      // gemm_rs6_* (bf16, six products), gemm_rs3_* (bf16, three), gemm_rs3h_* (fp16, three)
      static const char* const names[3][4] = {{"gemm_rs3_64x64", "gemm_rs3_256x256", "gemm_rs3_128x128", "gemm_rs3_128x64"},
                                              {"gemm_rs6_64x64", "gemm_rs6_256x256", "gemm_rs6_128x128", "gemm_rs6_128x64"},
                                              {"gemm_rs3h_64x64", "gemm_rs3h_256x256", "gemm_rs3h_128x128", "gemm_rs3h_128x64"}};
      return kind < 0 || kind > 2 ? "gemm_rs?" : names[kind][r.bm == 64 ? 0 : (r.bm == 256 ? 1 : (r.bn == 128 ? 2 : 3))];
    }
    case CONV_K_GEMM_SKINNY: return "gemm_skinny";
    case CONV_K_PW_256X256P: return "conv_pw_glds_256x256p";
    case CONV_K_PW_ARES: return "conv_pw_ares_128x128";
    case CONV_K_PW_256X256: return "conv_pw_glds_256x256";
    case CONV_K_PW_256X128P: return "conv_pw_glds_256x128p";
    case CONV_K_PW_256X128: return "conv_pw_glds_256x128";
    case CONV_K_PW_TILE: return ni == 0 ? "conv_pw_glds_128x128" : (ni == 1 ? "conv_pw_glds_128x64" : "conv_pw_glds_128x32");
    case CONV_K_PATCH:
      if (r.bk == 32) return r.bn == 64 ? "conv_patch_32x64s1" : "conv_patch_32x32s1";
      return r.stride == 1 ? "conv_patch_16x32s1" : "conv_patch_16x32s2";
    case CONV_K_PATCH_NCHW: return "conv_patch_nchw_16x32s2";
  }
  return "none";
}

}  // namespace peanut
