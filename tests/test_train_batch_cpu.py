"""Augmented training batches (ABI 25), the part that needs no GPU: ``TrainAugment``'s draws against the draws the reference's
pipeline made (tests/golden/train_batch_golden.npz), the float64 restatement of tests/train_batch_cases.py against the pipeline's
outputs and against scipy, what the cases claim about themselves (coverage, the tie condition), the pipeline reader's refusals, the
refusals of the C entry points, the binding and the header's words."""
import copy
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_batch_cases as tc                              # noqa: E402

from peanut_amd import _lib, mapio                          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -2
ALL_CASES = {**tc.OFF_CASES, **tc.ON_CASES}


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(tc.GOLDEN))


def _params(golden, name):
    p, d = golden[f"{name}/params"], golden[f"{name}/draws"]
    return [(int(a), int(b), int(f), int(r), float(ang)) for (a, b, f, r), ang in zip(p, d[:, 5])]


def test_the_golden_holds_the_cases_sequences_and_covers_what_the_gpu_tests_need(golden):
    assert mapio.rotation_terms(-142.137) == tc.rotation_terms(-142.137)
    for name, case in ALL_CASES.items():
        assert int(golden[f"{name}/seed"]) == case["seed"]
        for k, s in enumerate(tc.sequences(case)):
            assert s.dtype == np.uint8 and np.array_equal(golden[f"{name}/seq{k}"], s), name
        assert golden[f"{name}/img"].shape == (case["n"], case["C"]) + case["crop"]
        assert golden[f"{name}/gt"].shape == (case["n"], case["K"]) + case["crop"] and golden[f"{name}/gt"].any()
        assert max(case["map"] + case["pad"] + case["crop"]) <= 96
    assert all(not golden[f"{n}/params"][:, 3].any() and golden[f"{n}/img"].dtype == np.float32 for n in tc.OFF_CASES)
    assert all(golden[f"{n}/params"][:, 3].any() and golden[f"{n}/img"].dtype == np.float64 for n in tc.ON_CASES)
    tall, p = tc.OFF_CASES["tall"], golden["tall/params"]
    assert tall["crop"][0] > tall["map"][0]                                         # the crop is taller than the map
    mr, mc = tall["pad"][0] - tall["crop"][0], tall["pad"][1] - tall["crop"][1]
    assert {0, mr} <= set(p[:, 0].tolist()) and {0, mc} <= set(p[:, 1].tolist())    # offsets at 0 and at the full margin
    flips = set()
    for n in tc.OFF_CASES:
        flips |= set(golden[f"{n}/params"][:, 2].tolist())
    assert flips == {0, 1, 2}
    assert tc.OFF_CASES["tight"]["pad"] == tc.OFF_CASES["tight"]["map"] == tc.OFF_CASES["tight"]["crop"]
    assert tc.OFF_CASES["one"]["crop"] == (1, 1) and len(set(tc.OFF_CASES["m48"]["T"])) == 2
    some = golden["rot_some/params"][:, 3]
    assert some.any() and not some.all()                                            # rotate_prob < 1: both outcomes occur


@pytest.mark.parametrize("name", sorted(ALL_CASES))
def test_draws_equal_the_pipelines_bit_for_bit(golden, name):
    case = ALL_CASES[name]
    aug = mapio.TrainAugment.from_pipeline(tc.pipeline(case), seed=case["seed"])
    rows = aug.draw(case["n"], case["map"])
    assert rows.dtype == mapio.PARAMS_DTYPE
    want = golden[f"{name}/params"]
    for k, f in enumerate(("off_r", "off_c", "flip", "rotate")):
        assert np.array_equal(rows[f], want[:, k]), f
    assert rows["angle"].tobytes() == golden[f"{name}/draws"][:, 5].tobytes()       # the angle's bits, also where rotate is 0
    # a second call goes on in the stream; a fresh object with the seed starts over
    again = mapio.TrainAugment.from_pipeline(tc.pipeline(case), seed=case["seed"])
    both = np.concatenate([again.draw(3, case["map"]), again.draw(case["n"] - 3, case["map"])])
    assert both.tobytes() == rows.tobytes()


@pytest.mark.parametrize("name", sorted(ALL_CASES))
def test_restatement_equals_the_pipelines_outputs(golden, name):
    case, seqs = ALL_CASES[name], tc.sequences(ALL_CASES[name])
    for i, ((k, t), p) in enumerate(zip(tc.sample_sources(case), _params(golden, name))):
        r = tc.restate(seqs[k], t, *p, case["pad"], case["crop"], case["K"])
        want = golden[f"{name}/img"][i]
        if p[3]:
            assert np.abs(r["img"] - want).max() <= 1e-12, (name, i)
        else:
            assert np.array_equal(r["img"].astype(np.float32), want.astype(np.float32)) and np.array_equal(r["img"], want.astype(np.float64)), (name, i)
        assert np.array_equal(r["gt"], golden[f"{name}/gt"][i]), (name, i)


def _scipy_route(maps, t, off_r, off_c, flip, angle, pad, crop, K):
    """Pad, crop and flip with numpy, the rotation with scipy: independent of ``restate``'s taps."""
    from scipy.ndimage import affine_transform
    W, H = maps.shape[2:]
    Sr, Sc = crop
    img = (maps[t].astype(np.float32) / np.float32(255)).astype(np.float64)
    gt = maps[-1, 4:4 + K] * (maps[t, 1] == 0)
    out = []
    for a, order in ((img, 1), (gt, 0)):
        a = np.pad(a, [(0, 0), (0, pad[0] - W), (0, pad[1] - H)])[:, off_r:off_r + Sr, off_c:off_c + Sc]
        a = a[:, :, ::-1] if flip == 1 else a[:, ::-1] if flip == 2 else a
        c, s = tc.rotation_terms(angle)
        cy, cx = (Sr - 1) / 2.0, (Sc - 1) / 2.0
        off = [cy - c * cy + s * cx, cx - s * cy - c * cx]
        out.append(np.stack([affine_transform(np.ascontiguousarray(pl), [[c, -s], [s, c]], offset=off, order=order, mode="grid-constant", cval=0)
                             for pl in a]))
    return out


@pytest.mark.parametrize("shape", sorted(tc.ANGLE_SHAPES))
def test_restatement_agrees_with_scipy_and_no_case_has_a_tie(shape):
    sh = tc.ANGLE_SHAPES[shape]
    maps = tc.make_sequence(sh["T"], sh["C"], sh["map"], 77)
    for i, p in enumerate(tc.angle_params(tc.ANGLES, sh)):
        r = tc.restate(maps, i % sh["T"], *p, sh["pad"], sh["crop"], sh["K"])
        assert tc.tie_distance(r["near"]) > tc.TIE_MARGIN, (shape, p)
        img, gt = _scipy_route(maps, i % sh["T"], p[0], p[1], p[2], p[4], sh["pad"], sh["crop"], sh["K"])
        assert np.abs(r["img"] - img).max() <= 1e-12 and np.array_equal(r["gt"], gt), (shape, p)
        assert r["gt"].any() and r["img"].any()


def test_no_golden_case_has_a_tie_and_the_condition_sees_one(golden):
    for name, case in tc.ON_CASES.items():
        seqs = tc.sequences(case)
        for (k, t), p in zip(tc.sample_sources(case), _params(golden, name)):
            if p[3]:
                assert tc.tie_distance(tc.restate(seqs[k], t, *p, case["pad"], case["crop"], case["K"])["near"]) > tc.TIE_MARGIN
    # an even side at 45 degrees puts cells on a half-integer; odd sides, and even sides at these angles, do not
    maps = tc.make_sequence(2, 5, (16, 16), 1)
    tie = lambda crop, a: tc.tie_distance(tc.restate(maps, 0, 0, 0, 0, 1, a, (16, 16), crop, 1)["near"])
    assert tie((16, 16), 45.0) <= tc.TIE_MARGIN and tie((16, 16), 135.0) <= tc.TIE_MARGIN
    assert tie((15, 15), 45.0) > tc.TIE_MARGIN and tie((15, 13), 135.0) > tc.TIE_MARGIN
    for a in (1.0, 17.0, 30.0, 90.0, 180.0):
        assert tie((16, 16), a) > tc.TIE_MARGIN, a
    assert tie((16, 15), 90.0) <= tc.TIE_MARGIN                                      # sides of mixed parity at a right angle


def _reference_pipeline():
    return [
        dict(type="LoadMapFromFile"),
        dict(type="Resize", img_scale=None, ratio_range=(1.0, 1.0)),
        dict(type="Pad", size=(1200, 1200), pad_val=0, seg_pad_val=0),
        dict(type="RandomCrop", crop_size=(960, 960), cat_max_ratio=1.0),
        dict(type="RandomFlip", flip_ratio=0.5),
        dict(type="RandomRotate", prob=1.0, degree=180, pad_val=0, seg_pad_val=0),
        dict(type="DefaultFormatBundle"),
        dict(type="Collect", keys=["img", "gt_semantic_seg"]),
    ]


def test_from_pipeline_reads_the_references_list_and_refuses_what_is_not_built():
    aug = mapio.TrainAugment.from_pipeline(_reference_pipeline(), seed=5)       # nav/pred_model_cfg.py:47-56
    assert (aug.pad, aug.crop, aug.flip_prob, aug.flip_code, aug.rotate_prob, aug.degree) == ((1200, 1200), (960, 960), 0.5, 1, 1.0, (-180, 180))
    rows = aug.draw(4, (960, 960))
    assert rows["rotate"].all() and (np.abs(rows["angle"]) <= 180).all() and (rows["off_r"] <= 240).all()

    def edited(index, **fields):
        p = copy.deepcopy(_reference_pipeline())
        for k, v in fields.items():
            if v is _DROP:
                p[index].pop(k)
            else:
                p[index][k] = v
        return p
    bad = [
        edited(1, ratio_range=(0.5, 2.0)), edited(1, ratio_range=None), edited(1, img_scale=(960, 960)),
        edited(3, cat_max_ratio=0.75),
        edited(2, size=None, size_divisor=32), edited(2, size_divisor=32),
        edited(2, pad_val=1), edited(2, seg_pad_val=255), edited(2, seg_pad_val=_DROP),
        edited(5, seg_pad_val=255), edited(5, pad_val=0.5),
        edited(5, center=(10, 10)), edited(5, auto_bound=True),
        _reference_pipeline()[:5] + [dict(type="PhotoMetricDistortion")] + _reference_pipeline()[5:],
        [s for s in _reference_pipeline() if s["type"] != "RandomFlip"],
        _reference_pipeline()[:4] + [_reference_pipeline()[5], _reference_pipeline()[4]] + _reference_pipeline()[6:],
    ]
    for p in bad:
        with pytest.raises(ValueError):
            mapio.TrainAugment.from_pipeline(p)
    with pytest.raises(ValueError):
        aug.draw(1, (1201, 960))                                                  # a map larger than the pad: mmcv.impad asserts
    with pytest.raises(ValueError):
        mapio.TrainAugment(pad=(10, 10), crop=(11, 10))
    v = mapio.TrainAugment.from_pipeline(edited(4, direction="vertical"))
    assert v.flip_code == 2


_DROP = object()


def test_compact_sequence_keeps_the_chosen_frames_and_the_last():
    maps = tc.make_sequence(7, 10, (6, 5), 3)
    c = mapio.compact_sequence(maps, range(3))
    assert c.shape[0] == 4 and np.array_equal(c[:3], maps[:3]) and np.array_equal(c[-1], maps[-1]) and c.flags["C_CONTIGUOUS"]
    c = mapio.compact_sequence(maps, (4, 1))
    assert np.array_equal(c, maps[[4, 1, 6]])
    assert np.array_equal(mapio.target_from_sequence(c, 1), mapio.target_from_sequence(maps, 1))      # the maps[-1] convention
    with pytest.raises(ValueError):
        mapio.compact_sequence(maps, (7,))


def test_abi_25_binds_the_two_calls_and_their_descriptors():
    assert _lib.ABI_VERSION >= 25
    lib = _lib.load()
    assert lib.peanut_abi_version() == _lib.ABI_VERSION
    for name in ("peanut_mapseq_train_batch", "peanut_mapseq_bce_dense"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert C.sizeof(_lib.MapSeqAugC) == 48 and C.sizeof(_lib.MapSeqTrainC) == 8 + 10 * 4 + 4 * 8 and C.sizeof(_lib.MapSeqBceDenseC) == 8 + 4 * 4 + 4 * 8
    src = open(os.path.join(ROOT, "include", "peanut_hip.h"), encoding="utf-8").read()
    assert re.search(r"typedef struct \{\s*const uint8_t\* maps;\s*int32_t T, t_idx, off_r, off_c, flip, rotate;\s*double cos_t, sin_t;\s*\} peanut_mapseq_aug_t;", src)
    body = re.search(r"typedef struct \{([^}]*)\} peanut_mapseq_train_t;", src).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"[A-Za-z_]+(?=\s*[,;])", body) == [f for f, _ in _lib.MapSeqTrainC._fields_]      # the layout the binding mirrors
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{([^}]*)\} peanut_mapseq_bce_dense_t;", src).group(1), flags=re.S)
    assert re.findall(r"[A-Za-z_]+(?=\s*[,;])", body) == [f for f, _ in _lib.MapSeqBceDenseC._fields_]


def test_the_header_states_the_stream_class_of_the_two_calls():
    src = open(os.path.join(ROOT, "include", "peanut_hip.h"), encoding="utf-8").read()
    for symbol, pattern, desc in (("peanut_mapseq_train_batch", r"No\s+synchronisation", "peanut_mapseq_train_t"),
                                  ("peanut_mapseq_bce_dense", r"Synchronises", "peanut_mapseq_bce_dense_t")):
        at = src.index(f"int {symbol}(")
        own = src[src.rindex("\n/* ", 0, at):at]
        assert re.search(pattern, own), symbol
        assert "void* stream" not in src[at:src.index(";", at)]
        assert re.search(r"void\* stream;\s*\} " + desc + ";", src)


@pytest.mark.parametrize("what", sorted(tc.REFUSALS))
def test_train_batch_refuses_before_it_touches_the_device(what):
    lib = _lib.load()
    assert lib.peanut_mapseq_train_batch(C.byref(tc.train_desc(**tc.REFUSALS[what]))) == EINVAL, what
    assert lib.peanut_last_error()
    assert lib.peanut_mapseq_train_batch(None) == EINVAL


def test_bce_dense_refuses_before_it_touches_the_device():
    lib = _lib.load()
    out = (C.c_double * 4)()
    ok = dict(size=C.sizeof(_lib.MapSeqBceDenseC), B=1, K=2, S_r=6, S_c=6, logits=4096, gt=8192, sum_out=out, stream=None)
    for edit in (dict(size=16), dict(B=0), dict(B=65), dict(K=0), dict(S_r=0), dict(S_c=-1), dict(S_r=65536, S_c=65536), dict(logits=None),
                 dict(gt=None), dict(sum_out=None)):
        f = {**ok, **edit}
        d = _lib.MapSeqBceDenseC(f["size"], f["B"], f["K"], f["S_r"], f["S_c"], f["logits"], f["gt"], f["sum_out"], f["stream"])
        assert lib.peanut_mapseq_bce_dense(C.byref(d)) == EINVAL, edit
    assert lib.peanut_mapseq_bce_dense(None) == EINVAL
