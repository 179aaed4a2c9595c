"""The model-level policy options (csrc/options.h) no other test sets: which Winograd form a layer of the prediction net uploads and
runs (wino6_maxdil, wino5_mindil, wino_min_cin, wino_narrow_minpix), grouped against per-scale pyramid GEMMs (ppm_grouped), the
padding-row skip of the planner's position GEMMs (pw256_skip_pad), and the detector's forced front-end forms and plain stem
(rcnn_wino_m, rcnn_stem_s2d).

Every prediction-model setting is held to the committed reference goldens b2_96, odd_100 and rect_72x104 at the TOL of
tests/test_pred_gpu.py, and asserts BY OP NAME (``profile()``) that the plan is another one than the default handle's.  The golden
maps are too small for some of the changes -- all their Winograd layers pad to one GEMM tile per position, where F(4x4) always wins
-- so those settings also run the smallest input that shows the change, four 144 x 144 maps (18 x 18 features: the dilation-2 layers
take F(6x6), the dilation-4 layers F(5x5) by default), against oracle/pspnet_ref.forward_batch."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 5e-5           # tests/test_pred_gpu.py
GOLDEN_CASES = ("b2_96", "odd_100", "rect_72x104")
BIG = (4, 144, 144)
MANY = (11, 64, 64)  # eleven maps: 396 rows in the largest pyramid scale, where the size rule declines the grouped launch


@pytest.fixture(scope="module")
def pred():
    """Seeded weights (the goldens' seed), the golden inputs / logits, and the oracle's logits of the two extra inputs: made once."""
    from oracle import pspnet_ref
    from peanut_amd.weights import PredCfg, make_seeded_state_dict
    cfg = PredCfg()
    sd = make_seeded_state_dict(cfg, 0)
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pspnet_golden.npz"))
    golden = {}
    for case in GOLDEN_CASES:
        assert int(z[f"{case}/c_in"]) == cfg.in_channels and int(z[f"{case}/weight_seed"]) == 0
        golden[case] = (torch.from_numpy(z[f"{case}/input"].astype(np.float32)), torch.from_numpy(z[f"{case}/logits"]))
    extra = {}
    for shape in (BIG, MANY):
        g = torch.Generator().manual_seed(shape[0] * 1000 + shape[1])
        x = (torch.rand((shape[0], cfg.in_channels, shape[1], shape[2]), generator=g) > 0.7).float()
        extra[shape] = (x, pspnet_ref.forward_batch(sd, x, cfg))
    return SimpleNamespace(cfg=cfg, sd=sd, golden=golden, extra=extra, models={})


def _model(pred, options=None, precision=None):
    from peanut_amd.prediction import PEANUT_Prediction_Model
    key = (tuple(sorted((options or {}).items())), precision)
    if key not in pred.models:
        pred.models[key] = PEANUT_Prediction_Model(SimpleNamespace(sem_gpu_id=0), state_dict=pred.sd, cfg=pred.cfg, precision=precision,
                                                   options=options)
    return pred.models[key]


def _names(m, x):
    return [n for n, *_ in m.model.profile(x.cuda())]


def _goldens(pred, m, what, tol=TOL):
    worst = 0.0
    for case, (x, ref) in pred.golden.items():
        got = m.get_prediction_batch(x.cuda(), apply_sigmoid=False).cpu()
        err = (got - ref).abs().max().item()
        worst = max(worst, err)
        assert err <= tol, f"{what} {case}: max err {err:.3e}"
    print(f"{what}: max-abs vs the reference golden logits {worst:.3e} (bound {tol:.1e})")
    return worst


def _oracle(pred, m, shape, what, tol=TOL):
    x, ref = pred.extra[shape]
    got = m.get_prediction_batch(x.cuda(), apply_sigmoid=False).cpu()
    err = (got - ref).abs().max().item()
    print(f"{what} {shape}: max-abs vs the oracle's logits {err:.3e} (bound {tol:.1e})")
    assert err <= tol, f"{what} {shape}: max err {err:.3e}"
    return err


def _form(names, layer):
    """'wino6' / 'wino5' / 'wino' (F(4x4)) / 'direct': how the plan runs `layer`."""
    gemm = [n for n in names if n.startswith(layer + "[") and n.endswith("_gemm]")]
    if not gemm:
        assert layer in names, (layer, [n for n in names if n.startswith(layer)])
        return "direct"
    assert len(gemm) == 1, gemm
    return gemm[0][len(layer) + 1:-len("_gemm]")]


DIL2, DIL4, L1, L2 = "backbone.layer3.1.conv2", "backbone.layer4.1.conv2", "backbone.layer1.0.conv2", "backbone.layer2.1.conv2"


def test_default_plan_of_the_four_maps_has_all_three_forms(pred):
    """The ground the other cases stand on: at default options four 144 x 144 maps run layer3's dilation-2 convs as F(6x6), layer4's
    dilation-4 convs as F(5x5), layer2 as F(4x4) and layer1's 64-channel convs on the direct kernel; the golden maps run F(4x4)
    throughout.  The size rule of the pyramid takes the grouped launch for one map and declines it for eleven."""
    m = _model(pred)
    names = _names(m, pred.extra[BIG][0])
    assert (_form(names, DIL2), _form(names, DIL4), _form(names, L2), _form(names, L1)) == ("wino6", "wino5", "wino", "direct")
    for case, (x, _) in pred.golden.items():
        names = _names(m, x)
        assert (_form(names, DIL2), _form(names, DIL4), _form(names, L2), _form(names, L1)) == ("wino", "wino", "wino", "direct"), case
    one, many = _names(m, pred.golden["odd_100"][0]), _names(m, pred.extra[MANY][0])
    assert "decode_head.psp_modules.*.1.conv" in one and "decode_head.psp_modules.0.1.conv" not in one
    assert "decode_head.psp_modules.0.1.conv" in many and "decode_head.psp_modules.*.1.conv" not in many
    _goldens(pred, m, "default options")
    _oracle(pred, m, BIG, "default options")
    _oracle(pred, m, MANY, "default options")


def test_wino6_maxdil_1_keeps_dilated_layers_on_f4(pred):
    """wino6_maxdil = 1 (create-time): layers of dilation 2 and 4 upload the F(4x4) form alone.  On the four maps layer3 / layer4
    fall back from F(6x6) / F(5x5) to F(4x4) -- no larger-tile op is left in the plan -- and the logits hold the oracle; the goldens
    (F(4x4) either way) hold their bound."""
    m = _model(pred, {"wino6_maxdil": 1})
    names = _names(m, pred.extra[BIG][0])
    assert _form(names, DIL2) == "wino" and _form(names, DIL4) == "wino" and _form(names, "backbone.layer4.0.conv2") == "wino"
    assert not [n for n in names if "[wino6_" in n or "[wino5_" in n]
    _oracle(pred, m, BIG, "wino6_maxdil=1")
    _goldens(pred, m, "wino6_maxdil=1")


@pytest.mark.parametrize("mindil", [1, 0])
def test_wino5_mindil_moves_the_f5_form(pred, mindil):
    """wino5_mindil (create-time) = 1: every backbone layer also uploads F(5x5), and layer3's dilation-2 convs take it on the four
    maps (49 positions of one GEMM tile against 64); = 0: no layer has it, and layer4's dilation-4 convs run F(6x6) instead."""
    m = _model(pred, {"wino5_mindil": mindil})
    names = _names(m, pred.extra[BIG][0])
    if mindil == 1:
        assert _form(names, DIL2) == "wino5" and _form(names, DIL4) == "wino5"
    else:
        assert _form(names, DIL2) == "wino6" and _form(names, DIL4) == "wino6"
        assert not [n for n in names if "[wino5_" in n]
    _oracle(pred, m, BIG, f"wino5_mindil={mindil}")
    _goldens(pred, m, f"wino5_mindil={mindil}")


def test_wino_min_cin_256_takes_the_winograd_form_from_layer2(pred):
    """wino_min_cin = 256 (create-time): the 128-channel convs of layer2 carry no Winograd form and run the direct kernel at every
    size -- visible on the goldens themselves -- while layer3 (256 channels) keeps its forms."""
    m = _model(pred, {"wino_min_cin": 256})
    for case, (x, _) in pred.golden.items():
        names = _names(m, x)
        assert _form(names, L2) == "direct" and _form(names, "backbone.layer2.3.conv2") == "direct", case
        assert _form(names, DIL2) == "wino" and not [n for n in names if n.startswith("backbone.layer2.") and "[wino" in n], case
    _goldens(pred, m, "wino_min_cin=256")
    names = _names(m, pred.extra[BIG][0])
    assert _form(names, L2) == "direct" and _form(names, DIL2) == "wino6"
    _oracle(pred, m, BIG, "wino_min_cin=256")


def test_wino_narrow_minpix_1_runs_layer1_as_winograd_on_small_maps(pred):
    """wino_narrow_minpix = 1 (run-time; default 20 000 input pixels): layer1's 64-channel conv2 takes its Winograd form on the
    golden maps (24 x 24 features and smaller); set on a live handle, the plans are rebuilt."""
    m = _model(pred, {"wino_narrow_minpix": 1})
    for case, (x, _) in pred.golden.items():
        names = _names(m, x)
        assert _form(names, L1) == "wino" and _form(names, "backbone.layer1.2.conv2") == "wino", case
    _goldens(pred, m, "wino_narrow_minpix=1")
    _oracle(pred, m, BIG, "wino_narrow_minpix=1")
    assert _form(_names(m, pred.extra[BIG][0]), L1) != "direct"
    from peanut_amd.prediction import PEANUT_Prediction_Model
    live = PEANUT_Prediction_Model(SimpleNamespace(sem_gpu_id=0), state_dict=pred.sd, cfg=pred.cfg)
    x = pred.golden["b2_96"][0]
    assert _form(_names(live, x), L1) == "direct"
    live.model.set_option("wino_narrow_minpix", 1)
    assert _form(_names(live, x), L1) == "wino"
    assert torch.equal(live.get_prediction_batch(x.cuda(), apply_sigmoid=False), m.get_prediction_batch(x.cuda(), apply_sigmoid=False))


def test_wino_min_cin_64_gives_the_three_product_modes_layer1s_winograd_form(pred):
    """wino_min_cin = 64 is the planner's own floor in fp32 and bf16x6 (nothing would change there); in the three-product modes the
    floor is 128 (net_common.h: wino_eligible), so in fp16x3 the option is what gives layer1's 64-channel convs a Winograd form at
    all.  With the pixel gate open (wino_narrow_minpix = 1) on both handles: layer1 conv2 runs as Winograd only under
    wino_min_cin = 64.  fp16x3 is held to the goldens at the same 5e-5 (test_split_precision_forward_within_contract)."""
    opened = _model(pred, {"wino_narrow_minpix": 1}, precision="fp16x3")
    m = _model(pred, {"wino_narrow_minpix": 1, "wino_min_cin": 64}, precision="fp16x3")
    for case, (x, _) in pred.golden.items():
        assert _form(_names(opened, x), L1) == "direct", case
        assert _form(_names(m, x), L1) == "wino", case
    _goldens(pred, m, "fp16x3 wino_min_cin=64")
    _goldens(pred, opened, "fp16x3 wino_min_cin=0")
    _oracle(pred, m, BIG, "fp16x3 wino_min_cin=64")


def test_ppm_grouped_forced_against_the_size_rule(pred):
    """ppm_grouped = 0 on one map, where the rule takes the grouped launch: the four per-scale convs and Q tables run one by one;
    ppm_grouped = 1 on eleven 64 x 64 maps, where the rule declines (4 x 512 padded rows against 896 in separate launches -- six
    maps, 4 x 256 against 640, are still inside its factor of two): one grouped launch each with 512-row groups.  Op names tell the
    two apart.  The per-scale form holds the goldens (every case, batch 1 and 2), the forced grouped form the oracle's logits."""
    off = _model(pred, {"ppm_grouped": 0})
    for case, (x, _) in pred.golden.items():
        names = _names(off, x)
        assert [n for n in names if n.startswith("decode_head.psp_modules.") and n.endswith(".1.conv")] == \
            [f"decode_head.psp_modules.{i}.1.conv" for i in range(4)], case
        assert [n for n in names if n.startswith("decode_head.bottleneck.conv[ppm")] == [f"decode_head.bottleneck.conv[ppm{i}]" for i in range(4)], case
    _goldens(pred, off, "ppm_grouped=0")
    on = _model(pred, {"ppm_grouped": 1})
    names = _names(on, pred.extra[MANY][0])
    assert "decode_head.psp_modules.*.1.conv" in names and "decode_head.bottleneck.conv[ppm*]" in names
    assert not [n for n in names if n.startswith("decode_head.psp_modules.0")]
    _oracle(pred, on, MANY, "ppm_grouped=1")
    _oracle(pred, off, MANY, "ppm_grouped=0")
    _goldens(pred, on, "ppm_grouped=1")
    six = pred.extra[MANY][0][:6].contiguous()
    assert "decode_head.psp_modules.*.1.conv" in _names(_model(pred), six), "six maps are grouped by the size rule itself"


SKIP_PAD_OPTS = {"pw256_mink": 256, "pw256_mintiles": 1, "wino6_maxdil": 1}


def test_pw256_skip_pad_0_computes_the_padding_rows_of_the_position_groups(pred):
    """The 256 x 128 kernel skips the MFMAs of a wave whose 64 rows are all group padding only when the launch says how many rows of
    a group hold data (ConvArgs::group_valid_rows -> p.group_valid), which the prediction planner does for its Winograd position
    GEMMs (an operator-level conv handle does not, so the switch is inert there).  With the kernel's gates lowered and the
    dilation-2 layers on F(4x4) (wino6_maxdil = 1), four 144 x 144 maps give layer3.1-5 / layer4.0 conv2 4 x 4 x 9 = 144 tiles per
    position in one 256-row GEMM tile: the wave band of rows 192..255 is all padding.  Asserted from profile(): those position GEMMs
    run conv_pw_glds_256x128 under both settings.  pw256_skip_pad = 0 multiplies the zero rows instead; the data rows are computed
    by the same waves in the same order, so the logits must be equal bit for bit, and both hold the oracle (the option changes work
    done, not a result -- nothing else is observable)."""
    x = pred.extra[BIG][0]
    outs = []
    for skip in (1, 0):
        m = _model(pred, {**SKIP_PAD_OPTS, "pw256_skip_pad": skip})
        kern = {n: k for n, k, *_ in m.model.profile(x.cuda())}
        for layer in (DIL2, "backbone.layer3.5.conv2", "backbone.layer4.0.conv2"):
            assert kern[layer + "[wino_gemm]"] == "conv_pw_glds_256x128", (skip, layer, kern[layer + "[wino_gemm]"])
        _oracle(pred, m, BIG, f"pw256_skip_pad={skip} (position GEMMs on conv_pw_glds_256x128)")
        outs.append(m.get_prediction_batch(x.cuda(), apply_sigmoid=False))
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), f"{(outs[0] != outs[1]).sum().item()} logits differ"
    kern = {n: k for n, k, *_ in _model(pred, {"wino6_maxdil": 1}).model.profile(x.cuda())}
    assert kern[DIL2 + "[wino_gemm]"] != "conv_pw_glds_256x128"      # (without the lowered gates the layer is elsewhere: the gates are what brings it here)


# ---- detector ----
FRONT_TOL = 2e-5     # tests/test_rcnn_gpu.py: relative to 1 + max|ref|


@pytest.fixture(scope="module")
def det():
    from oracle import rcnn_ref
    from peanut_amd.rcnn import MaskRCNN
    from rcnn_cases import small_inputs
    cfg, sd, img = small_inputs()
    ref = rcnn_ref.forward_front(sd, img, cfg)
    base = MaskRCNN(cfg, sd)
    front = base.forward_front(img.cuda())
    return SimpleNamespace(cfg=cfg, sd=sd, img=img, ref=ref, base=base, front=[[t.clone() for t in ts] for ts in front],
                           detections=base.inference(img.cuda()), fronts={})


def _detector(det, **options):
    from peanut_amd import _lib
    from peanut_amd.rcnn import MaskRCNN
    with _lib.default_options(**options):
        return MaskRCNN(det.cfg, det.sd)


def _check_detector(det, m, what):
    """Pyramid, objectness and deltas against oracle/rcnn_ref.forward_front at FRONT_TOL; the detections of `inference` equal to the
    default handle's: same classes, scores within 1e-4, boxes within 0.05 px (test_inference_end_to_end's bounds)."""
    ref_p, ref_o, ref_d = det.ref
    img = det.img.cuda()
    pyr, obj, dl = m.forward_front(img)
    worst = 0.0
    for i, k in enumerate(("p2", "p3", "p4", "p5", "p6")):
        for name, got, ref in ((k, pyr[i], ref_p[k]), (f"obj{i}", obj[i], ref_o[i]), (f"delta{i}", dl[i], ref_d[i])):
            got = got.permute(0, 3, 1, 2).cpu()
            assert got.shape == ref.shape, name
            err = (got - ref).abs().max().item() / (1 + ref.abs().max().item())
            worst = max(worst, err)
            assert err <= FRONT_TOL, f"{what} {name}: {err:.3e} relative to 1 + max|ref|"
    print(f"{what}: front end worst error relative to 1 + max|ref| {worst:.3e} (bound {FRONT_TOL:.1e})")
    got = m.inference(img)
    assert len(got) == len(det.detections) == 2
    for g, r in zip(got, det.detections):
        assert len(r["scores"]) > 0
        assert g["pred_classes"].cpu().tolist() == r["pred_classes"].cpu().tolist(), what
        assert (g["scores"] - r["scores"]).abs().max().item() <= 1e-4, what
        assert (g["pred_boxes"] - r["pred_boxes"]).abs().max().item() <= 5e-2, what
    return [[t.clone() for t in ts] for ts in (pyr, obj, dl)]


def _front_bits_equal(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for xs, ys in zip(a, b) for x, y in zip(xs, ys))


def _pinned_front(det, tile):
    """Front-end outputs of a handle created under rcnn_wino_m = tile, made once per module (det.fronts)."""
    if tile not in det.fronts:
        pyr, obj, dl = _detector(det, rcnn_wino_m=tile).forward_front(det.img.cuda())
        det.fronts[tile] = [[t.clone() for t in ts] for ts in (pyr, obj, dl)]
    return det.fronts[tile]


@pytest.mark.parametrize("tile", [4, 5, 6])
def test_rcnn_wino_m_pins_one_form_in_the_front_end(det, tile):
    """rcnn_wino_m = 4 / 5 / 6 (create-time) on the small detector's two 96 x 128 frames: the front end against the restatement, the
    detections against the default handle's.  The op table names a Winograd op by its GEMM's kernel, not by its tile, so that the
    form was pinned shows in the arithmetic: this handle's pyramid, objectness and deltas differ in some bit from those of handles
    pinned to each of the other two forms (made here if no other case has made them yet), while a second handle of the same setting
    returns the same bits."""
    m = _detector(det, rcnn_wino_m=tile)
    fam = [k for _, k, _, _ in m.probe_front(det.img.cuda(), reps=1)]
    assert any(k.startswith("wino+") for k in fam)
    front = _check_detector(det, m, f"rcnn_wino_m={tile}")
    assert _front_bits_equal(front, _pinned_front(det, tile))
    for other in (4, 5, 6):
        if other != tile:
            assert not _front_bits_equal(front, _pinned_front(det, other)), f"rcnn_wino_m = {tile} and {other} computed the same bits"


def test_rcnn_stem_s2d_0_runs_the_plain_7x7_stem(det):
    """rcnn_stem_s2d = 0 (create-time): no space-to-depth form of the stem is uploaded and the 7x7 stride-2 conv runs on the
    full-size preprocessed image.  Same products in another order, and both stems run conv_igemm under one op name -- so the
    changed path shows in the bits: the pyramid differs from the default handle's, which a second default handle reproduces
    exactly."""
    m = _detector(det, rcnn_stem_s2d=0)
    front = _check_detector(det, m, "rcnn_stem_s2d=0")
    assert _front_bits_equal(det.front, _detector(det).forward_front(det.img.cuda()))
    assert not _front_bits_equal(front, det.front)
    names = [(n, k) for n, k, _, _ in m.probe_front(det.img.cuda(), reps=1)]
    assert names[0][0] == "preprocess" and names[1][0] == "backbone.bottom_up.stem.conv1" and names[1][1].startswith("conv_igemm_"), names[:2]
