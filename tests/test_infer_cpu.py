"""Sliding-window and flip-averaged inference (ABI 24), the part that needs no GPU: the window grid of the library against a
restatement of the reference's loop, the descriptor's refusals, the config reader on written-out files, the order of the test-time
augmentations, what tests/golden/infer_golden.npz claims about itself, the binding and the header's words."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import infer_cases as ic                                    # noqa: E402

from peanut_amd import _lib, prediction as P                # noqa: E402
from peanut_amd import weights as W                         # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -2


# ---- the window grid ------------------------------------------------------------------------------------------------------------
CROPS = [(16, 16), (24, 32), (32, 24), (64, 64)]
STRIDES = [(8, 12), (16, 16), (16, 20), (40, 40)]            # (40, 40) exceeds three of the crops: pixels that no window covers


def test_slide_windows_match_the_reference_loop():
    covered = refused = 0
    for H in range(16, 71, 3):
        for Wd in range(16, 71, 3):
            for crop in CROPS:
                for stride in STRIDES:
                    wins, ny, nx = ic.windows(H, Wd, crop, stride)
                    if ic.count_matrix(H, Wd, crop, stride).min() == 0:      # the reference's assert (encoder_decoder.py:185)
                        with pytest.raises(_lib.PeanutHipError, match="no window covers"):
                            P.slide_windows(H, Wd, crop, stride)
                        refused += 1
                        continue
                    ys, xs, ch, cw = P.slide_windows(H, Wd, crop, stride)
                    assert (len(ys), len(xs)) == (ny, nx) and (ch, cw) == (min(crop[0], H), min(crop[1], Wd))
                    assert [(y, x, y + ch, x + cw) for y in ys for x in xs] == wins, (H, Wd, crop, stride)
                    covered += 1
    assert covered > 3000 and refused > 500


def test_the_cases_are_what_the_table_says():
    for name, want in ic.COUNTS.items():
        c = ic.CASES[name]
        assert set(np.unique(ic.count_matrix(c["H"], c["W"], c["crop"], c["stride"])).tolist()) == want
    grids = {n: P.slide_windows(c["H"], c["W"], c["crop"], c["stride"]) for n, c in ic.CASES.items()}
    assert grids["A"] == ([0, 16, 17], [0, 20, 21], 24, 32)                 # ragged last windows shifted back
    assert all(x % 4 == 0 for x in grids["B"][1]) and grids["B"][3] % 4 == 0 and ic.CASES["B"]["W"] % 4 == 0    # the vector path
    assert grids["C"] == ([0, 16, 17], [0, 16, 31], 16, 16)
    assert grids["D"] == ([0], [0, 12, 24, 36], 20, 24)                     # the small patch
    assert grids["E"] == ([0], [0], 40, 56)
    assert P.HipSegmentor.slide_windows(41, 53, (24, 32), (16, 20)) == grids["A"]


def _windows(d, H=41, Wd=53):
    return _lib.load().peanut_pred_infer_windows(C.byref(d), H, Wd, None, None, None, None)


def test_descriptor_refusals():
    ok = P.infer_descriptor("slide", (24, 32), (16, 20), (0, 1))
    assert _windows(ok) == 9
    assert _windows(P.infer_descriptor("whole", flips=(0, 2))) == 1
    def slide(crop=(24, 32), stride=(16, 20), flips=(0,), **kw):
        return P.infer_descriptor("slide", crop, stride, flips, **kw)
    bad = []
    for n in (0, 5, -1):
        d = slide(); d.n_augs = n; bad.append((d, "n_augs"))
    for code in (3, -1):
        d = slide(flips=(0, 1)); d.flip[1] = code; bad.append((d, "flip code"))
    bad.append((slide(max_batch=-1), "max_batch"))
    bad.append((slide(crop=(16, 32), stride=(20, 20)), "no window covers"))          # stride > crop: rows 16..19 lie in no window
    bad.append((slide(crop=(24, 16), stride=(16, 20)), "no window covers"))          # columns 16..19
    assert _windows(slide(stride=(25, 20))) == 6                                     # (the shifted last window can close the gap)
    bad.append((slide(crop=(16, 16), stride=(16, 1)), "PEANUT_INFER_MAX_GRID"))       # 53 - 16 + 1 = 38 columns of windows
    bad.append((slide(crop=(15, 32), stride=(8, 20)), "at least 16"))                # a window below the forward's minimum
    bad.append((slide(crop=(24, 0)), "crop_size and stride"))
    bad.append((slide(stride=(16, 0)), "crop_size and stride"))
    d = P.infer_descriptor("whole"); d.mode = 2; bad.append((d, "mode"))
    for d, words in bad:
        assert _windows(d) == EINVAL, words
        assert words in _lib.load().peanut_last_error().decode(), (words, _lib.load().peanut_last_error())
    # 32 windows on an axis are the most: 16 + 31 * 1 = 47 columns
    assert _windows(P.infer_descriptor("slide", (16, 16), (16, 1)), 16, 47) == 32
    assert _windows(P.infer_descriptor("slide", (16, 16), (16, 1)), 16, 48) == EINVAL
    # whole mode on an image below the forward's minimum
    assert _windows(P.infer_descriptor("whole"), 15, 53) == EINVAL
    assert _lib.load().peanut_pred_infer_windows(None, 41, 53, None, None, None, None) == EINVAL
    with pytest.raises(ValueError):
        P.infer_descriptor("slide")
    with pytest.raises(ValueError):
        P.infer_descriptor("tiles", (24, 32), (16, 20))


# ---- the config reader ----------------------------------------------------------------------------------------------------------
MODEL = ("norm_cfg = dict(type='BN', requires_grad=True)\n"
         "model = dict(type='EncoderDecoder', pretrained='open-mmlab://resnet50_v1c',\n"
         "    backbone=dict(type='ResNetV1c', depth=50, num_stages=4, out_indices=(0, 1, 2, 3), dilations=(1, 1, 2, 4),\n"
         "                  strides=(1, 2, 1, 1), norm_cfg=norm_cfg, norm_eval=False, style='pytorch', contract_dilation=True,\n"
         "                  in_channels=14),\n"
         "    decode_head=dict(type='PSPHead', in_channels=2048, in_index=3, channels=512, pool_scales=(1, 2, 3, 6),\n"
         "                     dropout_ratio=0.1, num_classes=6, norm_cfg=norm_cfg, align_corners=False),\n"
         "    train_cfg=dict(), test_cfg=TEST_CFG)\n")
PIPELINE = ("test_pipeline = [dict(type='LoadMapFromFile'),\n"
            "                 dict(type='MultiScaleFlipAug', img_scale=IMG_SCALE, img_ratios=IMG_RATIOS, FLIP\n"
            "                      transforms=[TRANSFORMS])]\n"
            "data = dict(samples_per_gpu=8, test=dict(type='SemMapDataset', pipeline=test_pipeline))\n")
STOCK_TRANSFORMS = "dict(type='Resize', keep_ratio=True), dict(type='ImageToTensor', keys=['img']), dict(type='Collect', keys=['img'])"
FLIP_TRANSFORMS = STOCK_TRANSFORMS.replace("dict(type='ImageToTensor'", "dict(type='RandomFlip'), dict(type='ImageToTensor'")


def _cfg_text(test_cfg="dict(mode='whole')", flip="flip=False,", transforms=STOCK_TRANSFORMS, img_scale="None", img_ratios="[1.0]",
              pipeline=True):
    text = MODEL.replace("TEST_CFG", test_cfg)
    if pipeline:
        text += PIPELINE.replace("IMG_SCALE", img_scale).replace("IMG_RATIOS", img_ratios).replace("FLIP", flip).replace("TRANSFORMS", transforms)
    return text


def _parse(tmp_path, **kw):
    p = tmp_path / "cfg.py"
    p.write_text(_cfg_text(**kw))
    return W.pred_cfg_from_file(str(p))


def test_the_stock_config_parses_to_the_default(tmp_path):
    """The model and test-pipeline entries of the stock nav/pred_model_cfg.py (test_cfg whole, flip=False, img_ratios [1.0])."""
    assert _parse(tmp_path) == W.PredCfg()
    assert _parse(tmp_path, pipeline=False) == W.PredCfg()               # a file without a data section: the stock pipeline
    d = W.PredCfg()
    assert (d.test_mode, d.crop_size, d.stride, d.augs) == ("whole", None, None, ((False, "horizontal"),))
    assert d.plain_inference and d.flip_codes == (0,)


def test_honoured_config_edits(tmp_path):
    c = _parse(tmp_path, test_cfg="dict(mode='slide', crop_size=(480, 480), stride=(320, 320))")
    assert (c.test_mode, c.crop_size, c.stride, c.augs) == ("slide", (480, 480), (320, 320), ((False, "horizontal"),))
    assert not c.plain_inference and c.flip_codes == (0,)
    c = _parse(tmp_path, test_cfg="dict(mode='slide', crop_size=[24, 32], stride=[16, 20])")
    assert (c.crop_size, c.stride) == ((24, 32), (16, 20))
    c = _parse(tmp_path, flip="flip=True,", transforms=FLIP_TRANSFORMS)
    assert c.augs == ((False, "horizontal"), (True, "horizontal")) and c.flip_codes == (0, 1) and not c.plain_inference
    c = _parse(tmp_path, flip="flip=True, flip_direction='vertical',", transforms=FLIP_TRANSFORMS)
    assert c.flip_codes == (0, 2)
    # flip_direction without flip has no effect (the reference warns): one unflipped image per direction
    c = _parse(tmp_path, flip="flip=False, flip_direction='vertical',")
    assert c.augs == ((False, "vertical"),) and c.flip_codes == (0,) and c.plain_inference
    c = _parse(tmp_path, img_ratios="1.0")                              # a bare float is wrapped into a list (test_time_aug.py:70-71)
    assert c == W.PredCfg()


def test_aug_order_for_one_and_two_directions(tmp_path):
    """test_time_aug.py:120-129: ``for flip in [False, True]: for direction in flip_direction`` -- no de-duplication."""
    one = _parse(tmp_path, flip="flip=True, flip_direction=['horizontal'],", transforms=FLIP_TRANSFORMS)
    assert one.augs == ((False, "horizontal"), (True, "horizontal"))
    two = _parse(tmp_path, flip="flip=True, flip_direction=['horizontal', 'vertical'],", transforms=FLIP_TRANSFORMS)
    assert two.augs == ((False, "horizontal"), (False, "vertical"), (True, "horizontal"), (True, "vertical"))
    assert two.flip_codes == ic.AUG_LISTS["two_dirs"] == (0, 0, 1, 2)
    rev = _parse(tmp_path, flip="flip=True, flip_direction=['vertical', 'horizontal'],", transforms=FLIP_TRANSFORMS)
    assert rev.flip_codes == (0, 0, 2, 1)
    off = _parse(tmp_path, flip="flip=False, flip_direction=['horizontal', 'vertical'],")
    assert off.flip_codes == (0, 0) and not off.plain_inference          # two unflipped images: aug_test sums and halves them


@pytest.mark.parametrize("kw, words", [
    (dict(test_cfg="dict(mode='slide')"), "crop_size and stride"),
    (dict(test_cfg="dict(mode='slide', crop_size=(24, 32))"), "crop_size and stride"),
    (dict(test_cfg="dict(mode='slide', crop_size=(24, 32), stride=(16, 0))"), "positive ints"),
    (dict(test_cfg="dict(mode='slide', crop_size=(24, 32, 3), stride=(16, 20))"), "positive ints"),
    (dict(test_cfg="dict(mode='slide', crop_size=480, stride=320)"), "positive ints"),       # the reference unpacks a pair
    (dict(test_cfg="dict(mode='tiles')"), "'whole' or 'slide'"),
    (dict(img_ratios="[0.5, 1.0]"), "img_ratios"),
    (dict(img_ratios="[1.0, 1.0]"), "img_ratios"),
    (dict(img_ratios="None", img_scale="(960, 960)"), "img_scale"),
    (dict(img_scale="(960, 960)"), "img_scale"),
    (dict(flip="flip=True,"), "RandomFlip"),
    (dict(flip="flip=True, flip_direction='diagonal',", transforms=FLIP_TRANSFORMS), "flip_direction"),
    (dict(transforms=STOCK_TRANSFORMS + ", dict(type='Normalize', mean=[0, 0, 0], std=[1, 1, 1], to_rgb=False)"), "Normalize"),
    (dict(transforms=STOCK_TRANSFORMS.replace("dict(type='Resize', keep_ratio=True)", "dict(type='Pad', size_divisor=32)")), "Pad"),
    (dict(transforms=STOCK_TRANSFORMS.replace("keep_ratio=True", "keep_ratio=False")), "keep_ratio"),
    (dict(flip="flip=True, flip_direction=['horizontal', 'vertical', 'horizontal'],", transforms=FLIP_TRANSFORMS), "at most 4"),
])
def test_refused_config_edits(tmp_path, kw, words):
    with pytest.raises(ValueError, match=words):
        _parse(tmp_path, **kw)


def test_a_pipeline_without_multiscaleflipaug_is_refused(tmp_path):
    p = tmp_path / "cfg.py"
    p.write_text(_cfg_text(pipeline=False) + "data = dict(test=dict(pipeline=[dict(type='LoadMapFromFile'), dict(type='Collect', keys=['img'])]))\n")
    with pytest.raises(ValueError, match="MultiScaleFlipAug"):
        W.pred_cfg_from_file(str(p))


# ---- the fixture ----------------------------------------------------------------------------------------------------------------
def test_the_goldens_are_far_from_the_plain_result():
    """Every golden lies at least 100 x TOL from whole_inference of the unflipped image (here: the oracle's, which the other
    fixtures hold to the reference within 1e-5), so a test at TOL tells a slide or flip result from the plain one -- but case E
    without a flip, which IS the plain result (one window): it equals it within TOL."""
    from oracle import pspnet_ref
    z = np.load(ic.GOLDEN)
    assert sorted(z.files) == sorted(ic.key(c, a, m) for c in ic.CASES for a in ic.AUG_LISTS for m in ("slide", "distance"))
    assert os.path.getsize(ic.GOLDEN) < 1_000_000
    cfg = W.PredCfg()
    sd = W.make_seeded_state_dict(cfg, 0)
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    for case, c in ic.CASES.items():
        x = ic.inputs(case)
        assert float(x.min()) == 0.0 and 0.9 < float(x.max()) < 1.0 and 0.25 < float((x > 0).float().mean()) < 0.35
        whole = pspnet_ref.forward_batch(sd, x, cfg).numpy()
        for name in ic.AUG_LISTS:
            y = z[ic.key(case, name)]
            assert y.dtype == np.float32 and y.shape == (c["B"], 6, c["H"], c["W"])
            dist = float(np.abs(y - whole).max())
            assert abs(dist - float(z[ic.key(case, name, "distance")])) <= 1e-4, (case, name)
            if (case, name) == ("E", "none"):
                assert dist <= ic.TOL
            else:
                assert dist >= 100 * ic.TOL, (case, name, dist)
        # the goldens of one case differ from each other as well
        names = list(ic.AUG_LISTS)
        for i, a in enumerate(names):
            for b in names[i + 1:]:
                assert float(np.abs(z[ic.key(case, a)] - z[ic.key(case, b)]).max()) >= 100 * ic.TOL, (case, a, b)


def test_the_rule_restated_in_torch_matches_the_goldens_on_the_oracle():
    """tests/infer_cases.py's ``staged_batch`` + ``combine`` (what the GPU file holds the library to, bit for bit) on the oracle's
    window logits against the reference's own slide + flip results: case A, the pipeline's two-direction list."""
    from oracle import pspnet_ref
    cfg = W.PredCfg()
    sd = W.make_seeded_state_dict(cfg, 0)
    c = ic.CASES["A"]
    wins = ic.windows(c["H"], c["W"], c["crop"], c["stride"])[0]
    flips = ic.AUG_LISTS["two_dirs"]
    staged = ic.staged_batch(ic.inputs("A"), wins, flips)
    assert staged.shape == (len(flips) * c["B"] * len(wins), 14, 24, 32)
    got = ic.combine(pspnet_ref.forward_batch(sd, staged, cfg), wins, flips, c["B"], c["H"], c["W"]).numpy()
    assert np.abs(got - np.load(ic.GOLDEN)[ic.key("A", "two_dirs")]).max() <= 1e-5


# ---- binding and header ---------------------------------------------------------------------------------------------------------
def test_abi_and_symbols():
    lib = _lib.load()
    assert _lib.ABI_VERSION >= 24 and lib.peanut_abi_version() == _lib.ABI_VERSION
    for name in ("peanut_pred_inference", "peanut_pred_infer_windows", "peanut_pred_inference_workspace_bytes", "peanut_pred_infer_gather",
                 "peanut_pred_infer_combine"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert C.sizeof(_lib.PredInferC) == 56 and _lib.PredInferC.stream.offset == 48
    assert (_lib.INFER_MAX_AUGS, _lib.INFER_MAX_GRID) == (4, 32)


def test_the_header_states_the_contract():
    with open(os.path.join(ROOT, "include", "peanut_hip.h"), encoding="utf-8") as f:
        src = f.read()
    at = src.index("int peanut_pred_inference(")
    own = src[src.rindex("\n/* ", 0, at):at]
    assert not re.search(r"\bSynchronises\b|\bSynchronous\b", own) and re.search(r"No\s+synchronisation", own)
    for words in ("encoder_decoder.py:155-201", ":249-256", ":273-291", "base.py:62-110", "test_time_aug.py:102-135", ":166-177",
                  "aug-major", "IEEE division", "identity"):
        assert words in own, words
    assert "void* stream" not in src[at:src.index(";", at)]                       # the stream travels in the descriptor
    assert re.search(r"void\* stream;\s*\} peanut_pred_infer_t;", src)
    assert "#define PEANUT_INFER_MAX_AUGS 4" in src and "#define PEANUT_INFER_MAX_GRID 32" in src
