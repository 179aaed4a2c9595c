"""The conv operators (FusedConv, through the C ABI) on maps with a side of 1, 2 or 3, with dilations that exceed the map and with
GEMMs of 1 ... 6 rows, against F.conv2d in float64 on the CPU: the 3x3 direct kernels (fp32 and the three emulated modes), the
LDS-patch kernel, the three Winograd forms (sub-grids without a pixel, one ragged tile) and the pointwise kernels.  Inputs, the
scale / shift / residual / ReLU plumbing and the tolerances are those of tests/test_conv_gpu.py; every case asserts the kernel
family it was written for (peanut_last_conv_kernel) and every test prints the worst error it measured."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_conv_gpu import RS_TAG, RS_TOL, _last_kernel, _rand      # noqa: E402  (shared helpers and tolerances)

pytestmark = pytest.mark.gpu

FP32_TOL = 2e-5                                  # fp32 direct and pointwise: |err| <= 2e-5 * (1 + |ref|)
WINO_TOL = {4: 1.5e-4, 5: 4e-4, 6: 4e-4}         # F(4x4) / F(5x5) / F(6x6), fp32-class products (bf16x3: 1.5e-3 for F(4x4))


def _layer(B, H, W, cin, cout, k, stride, pad, dil, relu, residual, seed, affine=True):
    """Random layer as tests/test_conv_gpu.py draws it (fp32 values) and its float64 reference: x NCHW, w OIHW, scale, shift,
    residual (NCHW or None), ref."""
    g = torch.Generator().manual_seed(seed)
    x = _rand((B, cin, H, W), g)
    w = _rand((cout, cin, k, k), g, (2.0 / (cin * k * k)) ** 0.5)
    scale = torch.rand(cout, generator=g) + 0.5 if affine else None
    shift = _rand((cout,), g, 0.1) if affine else None
    ref = F.conv2d(x.double(), w.double(), None, stride=stride, padding=pad, dilation=dil)
    if affine:
        ref = ref * scale.double()[None, :, None, None] + shift.double()[None, :, None, None]
    res = None
    if residual:
        res = _rand(tuple(ref.shape), g)
        ref = ref + res.double()
    if relu:
        ref = F.relu(ref)
    return x, w, scale, shift, res, ref


def _nhwc(t):
    return None if t is None else t.permute(0, 2, 3, 1).contiguous().cuda()


def _rel_err(y_nhwc, ref):
    """max of |err| / (1 + |ref|): the tests assert it against the relative tolerance."""
    y = y_nhwc.permute(0, 3, 1, 2).cpu().double()
    assert y.shape == ref.shape, (tuple(y.shape), tuple(ref.shape))
    assert bool(torch.isfinite(y).all())
    return ((y - ref).abs() / (1 + ref.abs())).max().item()


# ---- 3x3, direct kernels ----
DIRECT_CASES = [
    # (B, H, W, cin, cout, stride, dil), padding = dilation            relu, residual
    ((1, 1, 1, 16, 32, 1, 1), True, False),       # one pixel: only the centre tap is inside the image, one k-tile of 16
    ((2, 1, 7, 32, 64, 1, 1), True, False),       # one row
    ((2, 7, 1, 32, 64, 1, 1), False, True),       # one column
    ((1, 2, 2, 64, 128, 2, 1), True, False),      # stride 2 on 2 x 2: a single output pixel
    ((1, 3, 3, 256, 256, 1, 4), True, True),      # dilation 4 on 3 x 3: the centre tap only (layer4 at 17 x 23)
    ((1, 2, 5, 512, 512, 1, 2), False, False),    # dilation 2 on 2 x 5: no vertical tap, horizontal ones on three columns
    ((3, 1, 1, 128, 96, 2, 1), True, True),       # stride 2 on one pixel, cout = 96, M = 3
]


@pytest.mark.parametrize("precision", ["fp32", "bf16x6", "fp16x3", "bf16x3"])
def test_direct_3x3_on_maps_with_a_side_of_1_to_3(precision):
    """conv_igemm_* (fp32) and conv_rs* (the emulated modes) on the seven shapes."""
    from peanut_amd.ops import FusedConv
    tol = FP32_TOL if precision == "fp32" else RS_TOL[precision]
    family = "conv_igemm_" if precision == "fp32" else "conv_" + RS_TAG[precision]
    worst = (0.0, None)
    for case, relu, residual in DIRECT_CASES:
        B, H, W, cin, cout, s, d = case
        x, w, scale, shift, res, ref = _layer(B, H, W, cin, cout, 3, s, d, d, relu, residual, seed=sum(case) + 17)
        conv = FusedConv(w, scale, shift, stride=s, padding=d, dilation=d, relu=relu, precision=precision, conv_algo="direct")
        xd, rd = _nhwc(x), _nhwc(res)
        y = conv(xd, residual=rd)
        assert _last_kernel().startswith(family), (case, _last_kernel())
        assert torch.equal(y, conv(xd, residual=rd)), case
        err = _rel_err(y, ref)
        worst = max(worst, (err, case))
        assert err <= tol, f"{case} on {_last_kernel()}: {err:.3e}"
    print(f"3x3 direct {precision} ({family}*): worst relative error {worst[0]:.3e} at {worst[1]} (bound {tol})")


# ---- 3x3, LDS-patch kernel ----
PATCH_CASES = [
    # (B, H, W, cin, cout, stride), relu, family
    ((1, 1, 1, 32, 64, 1), True, "conv_patch_32x64s1"),        # one pixel in one 16 x 8 tile
    ((1, 1, 40, 14, 32, 2), True, "conv_patch_16x32s2"),       # one row under stride 2, 14 -> 16 channels: Wo = 20, two tiles
    ((1, 3, 2, 32, 32, 1), False, "conv_patch_32x32s1"),
    ((2, 2, 17, 16, 32, 1), True, "conv_patch_16x32s1"),       # 17 columns: one full tile and one of a single column
]


@pytest.mark.parametrize("case,relu,family", PATCH_CASES, ids=lambda c: "x".join(map(str, c)) if isinstance(c, tuple) else None)
def test_patch_kernel_on_maps_with_a_side_of_1_to_3(case, relu, family):
    """conv_patch_* (patch_mintiles = 1) against F.conv2d and, as tests/test_conv_gpu.py's patch test, within 1e-5 of the
    implicit-GEMM kernel (patch_mintiles = 0) on the same layer."""
    from peanut_amd.ops import FusedConv, round_up, to_nhwc_padded
    B, H, W, cin, cout, s = case
    x, w, scale, shift, _, ref = _layer(B, H, W, cin, cout, 3, s, 1, 1, relu, False, seed=sum(case) + 29)
    xd = to_nhwc_padded(x.cuda(), round_up(cin, 16))
    y = FusedConv(w, scale, shift, stride=s, padding=1, relu=relu, conv_algo="direct", options={"patch_mintiles": 1})(xd)
    assert _last_kernel().startswith("conv_patch_") and _last_kernel() == family, _last_kernel()
    y0 = FusedConv(w, scale, shift, stride=s, padding=1, relu=relu, conv_algo="direct", options={"patch_mintiles": 0})(xd)
    assert _last_kernel().startswith("conv_igemm_"), _last_kernel()
    diff = float((y - y0).abs().max())
    err = _rel_err(y, ref)
    print(f"{family} {case}: relative error {err:.3e} (bound {FP32_TOL}); against conv_igemm {diff:.3e} (bound 1e-5)")
    assert diff <= 1e-5, f"differs from conv_igemm by {diff:.3e}"
    assert err <= FP32_TOL, f"{err:.3e}"


# ---- 3x3, Winograd ----
WINO_CASES = [
    # (B, H, W, cin, cout, dil), residual and ReLU (or neither)
    ((1, 1, 1, 256, 256, 1), True),       # one pixel in one tile
    ((2, 2, 3, 128, 128, 2), False),      # dilation 2 on 2 x 3: sub-grids of one row, one of them with a single column
    ((1, 3, 1, 512, 64, 4), True),        # dilation 4 on 3 x 1: 13 of the 16 sub-grids hold no pixel
    ((3, 2, 2, 256, 320, 4), False),      # dilation 4 on 2 x 2, batch 3, cout not a tile multiple
    ((1, 1, 9, 256, 256, 2), True),       # one row: sub-grids of 5 and 4 columns
    ((1, 5, 2, 128, 192, 1), False),      # two columns, 5 rows: ragged under every tile size
]


@pytest.mark.parametrize("m", [4, 5, 6])
@pytest.mark.parametrize("precision", ["fp32", "bf16x6", "fp16x3"])
def test_winograd_on_maps_with_a_side_of_1_to_3(precision, m):
    """conv_algo = 'auto' with wino_m = 4 / 5 / 6.  The last launch the handle notes is the position GEMM: conv_pw_glds_* in fp32,
    gemm_rs* in the emulated modes -- a direct kernel's name there would mean the Winograd path did not run.  For m = 4 and 6
    the small-problem transforms forced on (wino_small_maxwg = 2^30) and off (0) must agree bit for bit."""
    from peanut_amd.ops import FusedConv
    tol = WINO_TOL[m]
    family = "conv_pw_glds_" if precision == "fp32" else "gemm_" + RS_TAG[precision]
    worst = (0.0, None)
    seen = set()
    for case, full in WINO_CASES:
        B, H, W, cin, cout, d = case
        x, w, scale, shift, res, ref = _layer(B, H, W, cin, cout, 3, 1, d, d, full, full, seed=sum(case) + 41 + m)
        xd, rd = _nhwc(x), _nhwc(res)
        conv = FusedConv(w, scale, shift, padding=d, dilation=d, relu=full, precision=precision, options={"wino_m": m})
        y = conv(xd, residual=rd)
        assert _last_kernel().startswith(family), (case, _last_kernel())
        seen.add(_last_kernel())
        assert torch.equal(y, conv(xd, residual=rd)), case
        err = _rel_err(y, ref)
        worst = max(worst, (err, case))
        assert err <= tol, f"{case} F({m}x{m}) {precision}: {err:.3e}"
        del conv
        if m in (4, 6):
            ys = []
            for maxwg in (1 << 30, 0):
                c2 = FusedConv(w, scale, shift, padding=d, dilation=d, relu=full, precision=precision,
                               options={"wino_m": m, "wino_small_maxwg": maxwg})
                ys.append(c2(xd, residual=rd))
                assert _last_kernel().startswith(family), (case, maxwg, _last_kernel())
                del c2
            assert torch.equal(ys[0], ys[1]), (case, float((ys[0] - ys[1]).abs().max()))
            assert _rel_err(ys[0], ref) <= tol, case
    print(f"Winograd F({m}x{m}) {precision}: worst relative error {worst[0]:.3e} at {worst[1]} (bound {tol}); position GEMMs on {sorted(seen)}")


# ---- pointwise, M = 1 ... 6 ----
PW_CASES = [
    # (B, H, W, cin, cout, stride), relu, residual, fp32 family
    ((1, 1, 1, 64, 256, 1), True, True, "conv_pw_glds_"),        # M = 1, layer1 conv3's form: residual + ReLU
    ((1, 1, 1, 2048, 512, 1), True, False, "conv_pw_glds_"),     # split-K over one row
    ((1, 1, 1, 16, 128, 1), False, False, "conv_igemm_"),        # a single k-tile of 16
    ((1, 1, 1, 48, 64, 1), True, False, "conv_igemm_"),          # K = 48: no whole 32-channel k-tiles
    ((1, 2, 3, 256, 512, 2), False, False, "conv_pw_glds_"),     # strided: output 1 x 2
    ((2, 1, 1, 512, 6, 1), False, False, "conv_pw_glds_"),       # cout = 6 (conv_seg): exact fp32 in every mode
]


@pytest.mark.parametrize("precision", ["fp32", "bf16x6", "fp16x3", "bf16x3"])
def test_pointwise_with_one_to_six_rows(precision):
    """1x1 layers whose GEMM has M = 1 ... 6 rows -- one ragged tile, split-K over fewer rows than a wave handles -- and the
    two-source form (1, 1, 2, 32 + 2048, 128): the source switches after the first k-tile."""
    from peanut_amd.ops import FusedConv
    tol = FP32_TOL if precision == "fp32" else RS_TOL[precision]
    rs = None if precision == "fp32" else "gemm_" + RS_TAG[precision]
    worst = (0.0, None)
    seen = {}
    for case, relu, residual, fp32_family in PW_CASES:
        B, H, W, cin, cout, s = case
        x, w, scale, shift, res, ref = _layer(B, H, W, cin, cout, 1, s, 0, 1, relu, residual, seed=sum(case) + 53)
        conv = FusedConv(w, scale, shift, stride=s, relu=relu, precision=precision)
        xd, rd = _nhwc(x), _nhwc(res)
        y = conv(xd, residual=rd)
        family = fp32_family if (rs is None or cout < 64) else rs       # a narrow 1x1 stays exact fp32 in the emulated modes
        assert _last_kernel().startswith(family), (case, _last_kernel())
        seen[case] = _last_kernel()
        assert torch.equal(y, conv(xd, residual=rd)), case
        err = _rel_err(y, ref)
        worst = max(worst, (err, case))
        assert err <= tol, f"{case} on {_last_kernel()}: {err:.3e}"
    B, H, W, c1, c2, cout = 1, 1, 2, 32, 2048, 128
    g = torch.Generator().manual_seed(61)
    xa, xb = _rand((B, c1, H, W), g), _rand((B, c2, H, W), g)
    w = _rand((cout, c1 + c2, 1, 1), g, (2.0 / (c1 + c2)) ** 0.5)
    scale = torch.rand(cout, generator=g) + 0.5
    shift = _rand((cout,), g, 0.1)
    ref = F.relu(F.conv2d(torch.cat([xa, xb], 1).double(), w.double()) * scale.double()[None, :, None, None]
                 + shift.double()[None, :, None, None])
    conv = FusedConv(w, scale, shift, relu=True, precision=precision)
    y = conv(_nhwc(xa), x2=_nhwc(xb))
    assert _last_kernel().startswith(rs or "conv_pw_glds_"), _last_kernel()
    seen["two sources"] = _last_kernel()
    err = _rel_err(y, ref)
    worst = max(worst, (err, "two sources"))
    assert err <= tol, f"two sources on {_last_kernel()}: {err:.3e}"
    print(f"pointwise {precision}: worst relative error {worst[0]:.3e} at {worst[1]} (bound {tol}); kernels {seen}")


@pytest.mark.parametrize("hw", [(1, 1), (1, 2)], ids=["1x1", "1x2"])
def test_one_hot_probe_on_a_map_of_one_or_two_pixels(hw):
    """tests/test_conv_gpu.py::test_conv_transpose_detecting on a 1 x 1 and a 1 x 2 map: asymmetric one-hot probes, exact."""
    from peanut_amd.ops import FusedConv
    H, W = hw
    cin, cout = 32, 64
    x = torch.zeros(1, cin, H, W)
    x[0, 3, 0, W - 1] = 1.0
    x[0, 17, 0, 0] = 2.0
    w = torch.zeros(cout, cin, 1, 1)
    w[40, 3] = 1.0
    w[9, 17] = 3.0
    ref = F.conv2d(x.double(), w.double())
    assert ref[0, 40, 0, W - 1] == 1.0 and ref[0, 9, 0, 0] == 6.0 and int((ref != 0).sum()) == 2
    y = FusedConv(w)(_nhwc(x)).permute(0, 3, 1, 2).cpu()
    print(f"one-hot probe {H} x {W} on {_last_kernel()}")
    assert _last_kernel().startswith("conv_pw_glds_"), _last_kernel()
    assert torch.equal(y.double(), ref)
