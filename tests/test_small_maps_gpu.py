"""The prediction forward at the smallest maps it accepts (tests/small_map_cases.py: 16 x 16 ... 47 x 47 and the 16 x 720 strips,
a 2 x 2 ... 6 x 6 feature map or a 2 x 90 strip after the stride-8 backbone) against the oracle run in float64.

There the pyramid scales 3 and 6 exceed the feature map (adaptive-pool bins overlap or repeat pixels, the bilinear tables
DOWN-sample), dilations 2 and 4 exceed it (Winograd sub-grids without a pixel, direct kernels with only the centre tap inside),
every GEMM has one ragged row tile of 4 ... 36 rows, and the strips stress one axis only.  The tolerances are the suite's own
(tests/test_pred_gpu.py): 5e-5 on logits and sigmoid outputs for every fp32-class path, 5e-4 for bf16x3; the fp32 oracle itself
is within a quarter of that of the float64 run (tests/test_small_maps_cpu.py).  Every test prints the worst error it measured."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import small_map_cases as sm      # noqa: E402

pytestmark = pytest.mark.gpu

TOL = sm.TOL


def _model(align_corners=False, **kw):
    from peanut_amd.prediction import PEANUT_Prediction_Model
    cfg = sm.cfg_for(align_corners)
    return PEANUT_Prediction_Model(SimpleNamespace(sem_gpu_id=0), state_dict=sm.state_dict(cfg), cfg=cfg, **kw)


_XD = {}


def _xd(shape):
    """The case's input on the device (shared, never written to)."""
    if shape not in _XD:
        _XD[shape] = sm.inputs(shape).cuda()
    return _XD[shape]


def _logits(m, shape):
    return m.get_prediction_batch(_xd(shape), apply_sigmoid=False)


def _errors(m, shape):
    """(max-abs of the logits, max-abs of the sigmoid outputs) against the float64 oracle of the model's own cfg."""
    ref = sm.ref_logits(m.model.cfg, shape)
    got = _logits(m, shape).cpu().double()
    got_p = m.get_prediction_batch(_xd(shape), apply_sigmoid=True).cpu().double()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    return (got - ref).abs().max().item(), (got_p - torch.sigmoid(ref)).abs().max().item()


def _families(m, shape):
    """op name -> kernel family of one forward (the event probe's op table)."""
    return {n: k for n, k, *_ in m.model.profile(_xd(shape))}


@pytest.fixture(scope="module")
def default_model():
    m = _model()
    assert m.model.precision == "fp32" and m.model.conv_algo == "auto" and m.model.fold_ppm
    yield m
    del m


# ---- the default model: fp32, conv_algo auto, folded bottleneck ----

@pytest.mark.parametrize("shape", sm.SMALL_MAPS, ids=sm.shape_id)
def test_default_forward_matches_fp64_oracle(default_model, shape):
    m = default_model
    err, errp = _errors(m, shape)
    fam = _families(m, shape)
    gemms = sorted({n[n.index("["):] + "=" + k for n, k in fam.items() if "_gemm]" in n})
    print(f"{sm.shape_id(shape)} (layer4 {sm.LAYER4[shape]}): logits {err:.3e} sigmoid {errp:.3e} (bound {TOL}); stem.0 on "
          f"{fam['backbone.stem.0']}, pyramid term on {fam.get('ppm_conv_term')}, Winograd GEMMs {gemms}")
    assert err <= TOL, f"logits max err {err:.3e}"
    assert errp <= TOL, f"sigmoid max err {errp:.3e}"
    assert torch.equal(_logits(m, shape), _logits(m, shape))          # a repeated call is bit-identical


def test_default_forward_does_not_depend_on_batch_neighbours(default_model):
    """(9, 16, 16): map 4 among other neighbours (every other map all zeros or all ones) comes out bit for bit the same --
    same batch shape, same plan (tests/test_pred_gpu.py: test_batch_independence_and_determinism)."""
    m = default_model
    shape = (9, 16, 16)
    x = _xd(shape)
    full = _logits(m, shape).clone()
    y = x.clone()
    for i in range(9):
        if i != 4:
            y[i] = float(i % 2)
    assert torch.equal(y[4], x[4]) and not torch.equal(y[3], x[3])
    other = m.get_prediction_batch(y, apply_sigmoid=False)
    assert torch.equal(other[4], full[4])
    assert not torch.equal(other[3], full[3])


@pytest.mark.parametrize("shape", [(1, 16, 16), (2, 17, 23)], ids=sm.shape_id)
def test_taps_match_fp64_oracle(default_model, shape):
    """Every named intermediate of tests/test_pred_gpu.py::test_taps_match_oracle_96 against the float64 taps, TOL * max(1, scale):
    a failure names its stage."""
    m = default_model
    cfg = m.model.cfg
    ref = sm.ref_taps(cfg, shape)
    B = shape[0]
    worst = {}
    m.model.debug_keep(True)
    try:
        _logits(m, shape)
        torch.cuda.synchronize()
        for name in sm.TAP_NAMES:
            got = m.model.debug_tensor(name).permute(0, 3, 1, 2).contiguous().cpu().double()
            assert got.shape == ref[name].shape, name
            err = (got - ref[name]).abs().max().item()
            scale = ref[name].abs().max().item()
            worst[name] = err / max(1.0, scale)
            assert err <= TOL * max(1.0, scale), f"{name}: max err {err:.3e} (scale {scale:.2f})"
        # ppm_table is scale-major [scale][B][k*k][C]; the oracle gives [B,C,50]
        tbl = m.model.debug_tensor("ppm_table").cpu().double().reshape(-1, cfg.head_channels)
        row0 = col0 = 0
        for k in cfg.pool_scales:
            blk = tbl[row0:row0 + B * k * k].reshape(B, k * k, -1).permute(0, 2, 1)
            r = ref["ppm_table"][:, :, col0:col0 + k * k]
            err = (blk - r).abs().max().item()
            scale = r.abs().max().item()
            worst[f"ppm_table[{k}]"] = err / max(1.0, scale)
            assert err <= TOL * max(1.0, scale), f"ppm_table k={k}: max err {err:.3e} (scale {scale:.2f})"
            row0 += B * k * k
            col0 += k * k
    finally:
        m.model.debug_keep(False)
    name = max(worst, key=worst.get)
    print(f"{sm.shape_id(shape)}: worst tap {name} at {worst[name]:.3e} of max(1, scale) (bound {TOL})")


@pytest.mark.parametrize("shape", [(1, 16, 16), (2, 17, 23)], ids=sm.shape_id)
def test_graph_replay_is_bit_identical(default_model, shape):
    """The protocol of tests/test_pred_gpu.py::test_graph_replay_is_bit_identical on a side stream: first call direct, second
    captured, later ones replayed -- all bit-identical to the plain model; then the same input buffer with new contents."""
    m = default_model
    g = _model()
    g.model.use_graph(True)
    side = torch.cuda.Stream()
    x = _xd(shape).clone()
    want = m.get_prediction_batch(x, apply_sigmoid=True)
    out = torch.empty_like(want)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for rep in range(4):
            out.zero_()
            g.get_prediction_batch(x, apply_sigmoid=True, out=out)
            side.synchronize()
            assert torch.equal(out, want), (shape, rep)
        x2 = (torch.rand(tuple(x.shape), generator=torch.Generator().manual_seed(6)) > 0.7).float().cuda()
        assert not torch.equal(x2, x)
        x.copy_(x2)
        g.get_prediction_batch(x, apply_sigmoid=True, out=out)
        side.synchronize()
    want2 = m.get_prediction_batch(x2, apply_sigmoid=True)
    assert torch.equal(out, want2) and not torch.equal(want2, want)
    del g


def test_size_boundary(default_model):
    """15 is refused on either axis with a message, the handle then answers 16 x 16 as before; the size queries serve 16 x 16."""
    from peanut_amd import _lib
    m = default_model
    lib = _lib.load()
    shape = (1, sm.MIN_SIDE, sm.MIN_SIDE)
    before = _logits(m, shape).clone()
    c = m.model.cfg.in_channels
    for h, w in [(sm.BELOW_MIN, sm.MIN_SIDE), (sm.MIN_SIDE, sm.BELOW_MIN)]:
        with pytest.raises(_lib.PeanutHipError):
            m.get_prediction_batch(torch.zeros((1, c, h, w), device="cuda"))
        assert lib.peanut_last_error(), (h, w)
        assert torch.equal(_logits(m, shape), before), (h, w)
    assert m.model.workspace_bytes(1, sm.MIN_SIDE, sm.MIN_SIDE) > 0 and m.model.flops_per_map(sm.MIN_SIDE, sm.MIN_SIDE) > 0
    assert m.model.workspace_bytes(9, sm.MIN_SIDE, sm.MIN_SIDE) >= m.model.workspace_bytes(1, sm.MIN_SIDE, sm.MIN_SIDE)


# ---- variants on CORE, each against the float64 oracle of its own cfg ----

def _wino_tag(m):
    return "[wino_gemm]" if m == 4 else f"[wino{m}_gemm]"


VARIANTS = {
    # name: (model keywords, bound on logits and sigmoid)
    "plain_bottleneck": (dict(fold_ppm=False), TOL),
    "direct": (dict(conv_algo="direct"), TOL),
    "wino4": (dict(options={"wino_m": 4}), TOL),
    "wino5": (dict(options={"wino_m": 5}), TOL),
    "wino6": (dict(options={"wino_m": 6}), TOL),
    "patch": (dict(options={"patch_mintiles": 1}), TOL),
    "patch_nhwc": (dict(options={"patch_mintiles": 1, "stem_nchw": 0}), TOL),
    "no_patch": (dict(options={"patch_mintiles": 0}), TOL),
    "align_corners": (dict(align_corners=True), TOL),
    # the bounds of tests/test_pred_gpu.py::test_split_precision_forward_within_contract
    "bf16x3": (dict(precision="bf16x3"), 5e-4),
    "bf16x6": (dict(precision="bf16x6"), 5e-5),
    "fp16x3": (dict(precision="fp16x3"), 5e-5),
}
STEM0 = {"patch": "conv_patch_nchw_16x32s2", "patch_nhwc": "conv_patch_16x32s2", "no_patch": "conv_igemm_"}


@pytest.fixture(scope="module", params=list(VARIANTS))
def variant(request):
    """One handle per variant, built once for all its shapes and freed before the next variant's is built."""
    kw, tol = VARIANTS[request.param]
    m = _model(**kw)
    yield request.param, m, tol
    del m


@pytest.mark.parametrize("shape", sm.CORE, ids=sm.shape_id)
def test_variant_matches_fp64_oracle(variant, default_model, shape):
    name, m, tol = variant
    err, errp = _errors(m, shape)
    fam = _families(m, shape)
    note = ""
    if name == "plain_bottleneck":
        assert not m.model.fold_ppm and "ppm_conv_term" not in fam
        diff = (_logits(m, shape) - _logits(default_model, shape)).abs().max().item()
        note = f"; against the folded model {diff:.3e} (bound 5e-5)"
        assert diff <= 5e-5, f"plain vs folded bottleneck {diff:.3e}"
    elif name == "direct":
        assert not any("_gemm]" in n for n in fam), [n for n in fam if "_gemm]" in n]
        dil4 = [k for n, k in fam.items() if n.endswith("layer4.1.conv2")]
        assert dil4 and all(k.startswith("conv_igemm_") for k in dil4), dil4
        note = f"; layer4.1.conv2 (dilation 4) on {dil4}"
    elif name.startswith("wino"):
        tag = _wino_tag(int(name[4:]))
        gemms = [n for n in fam if "_gemm]" in n]
        # every shape here runs Winograd layers (layer2 ... layer4 conv2 and the bottleneck have >= 128 input channels): were
        # that to change, this fails instead of passing in silence
        assert gemms and all(n.endswith(tag) for n in gemms), (shape, gemms)
        assert any("bottleneck.conv[x]" in n for n in gemms) and any("layer4.1.conv2" in n for n in gemms), gemms
        note = f"; {len(gemms)} position GEMMs {tag} on {sorted({fam[n] for n in gemms})}"
    elif name in STEM0:
        stem = [fam["backbone.stem.0"], fam["backbone.stem.3"], fam["backbone.stem.6"]]
        assert stem[0].startswith(STEM0[name]), stem
        assert ("nchw_to_nhwc" in fam) == (name != "patch"), list(fam)[:3]
        if name == "no_patch":
            assert all(s.startswith("conv_igemm_") for s in stem), stem
        else:
            assert stem[1:] == ["conv_patch_32x32s1", "conv_patch_32x64s1"], stem
        note = f"; stem on {stem}"
    elif name == "align_corners":
        assert m.model.cfg.align_corners
        # not the same function as the default model: the case would pass on a handle that ignored the flag otherwise
        assert (_logits(m, shape) - _logits(default_model, shape)).abs().max().item() > TOL
    else:
        assert m.model.precision == name
        rs = sorted({k for k in fam.values() if k.startswith(("gemm_rs", "conv_rs"))})
        assert rs, sorted(set(fam.values()))
        note = f"; emulated kernels {rs}"
    print(f"{name} {sm.shape_id(shape)}: logits {err:.3e} sigmoid {errp:.3e} (bound {tol}){note}")
    assert err <= tol, f"{name}: logits max err {err:.3e}"
    assert errp <= tol, f"{name}: sigmoid max err {errp:.3e}"


# ---- pairs the code claims to be the same arithmetic ----

def test_pyramid_term_row_kernel_is_bit_identical():
    """ppm_term_rows 1 against 0 (csrc/pspnet_aux.hip: one wave per output row against the workgroup-wide two-phase kernel).  The
    row kernel's gate is (C / 32) * B >= 128, i.e. B >= 8 with 512 head channels: (9, 16, 16) is the case that reaches it, with
    2 feature rows for its 16 waves; the other shapes run the same kernel on both sides.  The op table names both kernels
    ppm_conv_term, so which one ran follows from the gate and is not asserted."""
    m1, m0 = _model(options={"ppm_term_rows": 1}), _model(options={"ppm_term_rows": 0})
    assert m1.model.get_option("ppm_term_rows") == 1 and m0.model.get_option("ppm_term_rows") == 0
    for shape in sm.CORE:
        a, b = _logits(m1, shape), _logits(m0, shape)
        assert torch.equal(a, b), (shape, float((a - b).abs().max()))
        gate = (m1.model.cfg.head_channels // 32) * shape[0] >= 128
        print(f"{sm.shape_id(shape)}: ppm_term_rows 1 on {_families(m1, shape)['ppm_conv_term']} (row-kernel gate "
              f"{'open' if gate else 'closed'}), 0 on {_families(m0, shape)['ppm_conv_term']}: bit-identical")
        err, errp = _errors(m1, shape)
        assert err <= TOL and errp <= TOL, (shape, err, errp)
    assert (m1.model.cfg.head_channels // 32) * 9 >= 128 > (m1.model.cfg.head_channels // 32) * 2
    del m1, m0


def test_small_problem_winograd_transforms_are_bit_identical():
    """wino_small_maxwg 2^30 (a workgroup per tile and channel slice, through LDS) against 0 (a thread per tile and channel
    group): the same helpers on the same operands, with sub-grids that hold no pixel at all."""
    ms, m0 = _model(options={"wino_small_maxwg": 1 << 30}), _model(options={"wino_small_maxwg": 0})
    for shape in sm.CORE:
        a, b = _logits(ms, shape), _logits(m0, shape)
        assert torch.equal(a, b), (shape, float((a - b).abs().max()))
        fam = _families(ms, shape)
        assert any("_gemm]" in n for n in fam), list(fam)
        err, errp = _errors(ms, shape)
        print(f"{sm.shape_id(shape)}: wino_small_maxwg 2^30 and 0 bit-identical; logits {err:.3e} sigmoid {errp:.3e} (bound {TOL})")
        assert err <= TOL and errp <= TOL, (shape, err, errp)
    del ms, m0


def test_pyramid_pooling_row_groups_match_the_row_pass():
    """ppm_group_rows 2 and 5 against 1 (csrc/pspnet_aux.hip: the row pass adds up groups of rows that share every scale's
    bin-row) where bins of scales 3 and 6 share rows or repeat them: the pooled table within 1e-6 * (1 + max|t|) of one row per
    workgroup, the logits within TOL of the float64 oracle (the bounds of
    tests/test_pred_gpu.py::test_pyramid_pooling_row_groups_match_the_row_pass)."""
    m1 = _model(options={"ppm_group_rows": 1})
    m1.model.debug_keep(True)
    t1 = {}
    for shape in sm.CORE:
        _logits(m1, shape)
        t1[shape] = m1.model.debug_tensor("ppm_table").cpu()
    for rows in (2, 5):
        mg = _model(options={"ppm_group_rows": rows})
        mg.model.debug_keep(True)
        for shape in sm.CORE:
            err, errp = _errors(mg, shape)
            tg = mg.model.debug_tensor("ppm_table").cpu()
            dt = float((tg - t1[shape]).abs().max())
            bound = 1e-6 * (1.0 + float(t1[shape].abs().max()))
            print(f"ppm_group_rows {rows} {sm.shape_id(shape)}: table against one row per workgroup {dt:.3e} (bound {bound:.3e}); "
                  f"logits {err:.3e} sigmoid {errp:.3e} (bound {TOL})")
            assert tg.shape == t1[shape].shape and dt <= bound, (rows, shape, dt)
            assert err <= TOL and errp <= TOL, (rows, shape, err, errp)
        del mg
    del m1
