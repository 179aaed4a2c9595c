"""Writes tests/golden/train_batch_golden.npz: what the reference's OWN training transforms -- ``Resize``, ``Pad``, ``RandomCrop``,
``RandomFlip``, ``RandomRotate`` (prediction/mmseg/datasets/pipelines/transforms.py, loaded unmodified by file path) -- make of the
samples of tests/train_batch_cases.py under ``np.random.seed(seed)``, and the random draws they made on the way.

``mmcv`` is not installed, so the file is loaded under a wiring-only stand-in (on top of oracle/ref_import.py's): ``impad`` is
``np.pad``, ``imflip`` is ``np.flip``, ``imrescale`` is the identity and asserts that the ratio is 1, ``imrotate`` applies the stated
rotation rule (mmcv.imrotate with center None and auto_bound False: ``cv2.getRotationMatrix2D(center, -angle, 1)`` and ``warpAffine``
without WARP_INVERSE_MAP, border constant) through ``scipy.ndimage.affine_transform(order=1 / 0, mode='grid-constant')`` in float64.
cv2's fixed-point coordinates (1/1024 px, fractions of 1/32 px) are therefore NOT in the fixtures: DESIGN.md states it.

``LoadMapFromFile`` (train_prediction_model.py:64-89) is restated in ``load_sample`` (it reads a file; here the sequence is in
memory).  The draws are captured by recording wrappers around ``np.random.uniform`` / ``rand`` / ``randint`` / ``random_sample``
that return what numpy returns.

The file holds data only, per case: ``<case>/seq<k>`` the uint8 sequences, ``<case>/seed``, ``<case>/draws`` float64 [n, 6]
(resize sample, off_r, off_c, flip rand, rotate rand, angle -- the angle's bits), ``<case>/params`` int32 [n, 4] (off_r, off_c,
flip code, rotate), ``<case>/img`` (float32 for the rotation-off cases, float64 for the rotation-on ones) and ``<case>/gt`` uint8.

Needs the reference checkout (it does not travel with the tests; the .npz does).

    python -m tools.gen_golden_train_batch
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import train_batch_cases as tc                                   # noqa: E402
from oracle import ref_import                                    # noqa: E402


def _imrotate(img, angle, center=None, scale=1.0, border_value=0, interpolation="bilinear", auto_bound=False):
    from scipy.ndimage import affine_transform
    assert center is None and not auto_bound and scale == 1.0
    h, w = img.shape[:2]
    cy, cx = (h - 1) * 0.5, (w - 1) * 0.5
    c, s = tc.rotation_terms(angle)
    matrix = np.array([[c, -s], [s, c]])
    offset = np.array([cy - c * cy + s * cx, cx - s * cy - c * cx])
    order = {"bilinear": 1, "nearest": 0}[interpolation]
    out = np.empty(img.shape, np.float64 if order else img.dtype)
    for k in range(img.shape[2]):
        src = img[:, :, k].astype(np.float64) if order else img[:, :, k]
        affine_transform(src, matrix, offset=offset, order=order, mode="grid-constant", cval=border_value, output=out[:, :, k])
    return out


def _impad(img, shape, pad_val=0):
    assert shape[0] >= img.shape[0] and shape[1] >= img.shape[1]
    width = [(0, shape[0] - img.shape[0]), (0, shape[1] - img.shape[1])] + [(0, 0)] * (img.ndim - 2)
    return np.pad(img, width, mode="constant", constant_values=pad_val)


def _imrescale(img, scale, return_scale=False, interpolation="bilinear"):
    h, w = img.shape[:2]
    factor = min(max(scale) / max(h, w), min(scale) / min(h, w))
    assert factor == 1.0, "only ratio 1 is built"
    return (img, factor) if return_scale else img


def _deprecated_api_warning(name_dict, cls_name=None):
    def deco(fn):
        def wrapped(*args, **kwargs):
            for old, new in name_dict.items():
                if old in kwargs:
                    kwargs[new] = kwargs.pop(old)
            return fn(*args, **kwargs)
        return wrapped
    return deco


def load_transforms():
    """The reference's transforms.py, unmodified, under the stand-in -> the module."""
    ref_import._install_mmcv_standin()
    mmcv = sys.modules["mmcv"]
    if getattr(mmcv, "_peanut_standin", False):
        mmcv.impad, mmcv.imrescale, mmcv.imrotate = _impad, _imrescale, _imrotate
        mmcv.imflip = lambda img, direction="horizontal": np.flip(img, axis=1 if direction == "horizontal" else 0)
        mmcv.is_list_of = lambda seq, typ: isinstance(seq, list) and all(isinstance(v, typ) for v in seq)
        mmcv.utils.deprecated_api_warning = _deprecated_api_warning
        mmcv.utils.is_tuple_of = lambda seq, typ: isinstance(seq, tuple) and all(isinstance(v, typ) for v in seq)
    for name in ("mmseg", "mmseg.datasets", "mmseg.datasets.pipelines"):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__path__ = []
            sys.modules[name] = m
    builder = types.ModuleType("mmseg.datasets.builder")
    builder.PIPELINES = sys.modules["mmcv"].utils.Registry("pipeline")
    sys.modules["mmseg.datasets.builder"] = builder
    path = os.path.join(ref_import.MMSEG, "datasets", "pipelines", "transforms.py")
    spec = importlib.util.spec_from_file_location("mmseg.datasets.pipelines.transforms", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod, builder.PIPELINES


def load_sample(maps, t_idx, K):
    """LoadMapFromFile.__call__ (train_prediction_model.py:64-91) on a sequence in memory."""
    img = maps[t_idx].transpose(1, 2, 0)
    img = img.astype(np.float32) / 255.
    mask = (img[:, :, 1] > 0)
    goals = range(4, 4 + K)
    gt = (maps[-1, goals] * (1 - mask)).transpose(1, 2, 0)
    return dict(img=img, img_shape=img.shape, ori_shape=img.shape, pad_shape=img.shape, scale_factor=1.0,
                gt_semantic_seg=gt, seg_fields=["gt_semantic_seg"])


class _Recorder:
    """Records what np.random's module-level draws return while the pipeline runs."""
    NAMES = ("random_sample", "randint", "rand", "uniform")

    def __enter__(self):
        self.log, self.saved = [], {}
        for name in self.NAMES:
            orig = getattr(np.random, name)
            self.saved[name] = orig

            def wrapped(*a, _orig=orig, _name=name, **k):
                v = _orig(*a, **k)
                self.log.append((_name, v))
                return v
            setattr(np.random, name, wrapped)
        return self

    def __exit__(self, *exc):
        for name, orig in self.saved.items():
            setattr(np.random, name, orig)
        return False


def run_case(registry, case):
    seqs = tc.sequences(case)
    transforms = [registry.build(cfg) for cfg in tc.pipeline(case) if cfg["type"] not in ("LoadMapFromFile", "DefaultFormatBundle", "Collect")]
    code = {"horizontal": 1, "vertical": 2}[case["direction"]]
    draws, params, imgs, gts = [], [], [], []
    np.random.seed(case["seed"])
    for k, t in tc.sample_sources(case):
        results = load_sample(seqs[k], t, case["K"])
        with _Recorder() as rec:
            for tr in transforms:
                results = tr(results)
        names = [n for n, _ in rec.log]
        assert names == ["random_sample", "randint", "randint", "rand", "rand", "uniform"], names
        v = [float(x) for _, x in rec.log]
        draws.append(v)
        flip = code if results["flip"] else 0
        rotate = int(v[4] < case.get("rotate_prob", 0.0))
        assert bool(results["flip"]) == (v[3] < tc.FLIP_PROB)
        params.append([int(v[1]), int(v[2]), flip, rotate])
        img = results["img"].transpose(2, 0, 1)
        imgs.append(img.astype(np.float64) if case.get("rotate_prob", 0.0) > 0 else img.astype(np.float32))
        gts.append(np.ascontiguousarray(results["gt_semantic_seg"].transpose(2, 0, 1)).astype(np.uint8))
        assert imgs[-1].shape == (case["C"],) + tuple(case["crop"]) and gts[-1].shape == (case["K"],) + tuple(case["crop"])
    return seqs, np.array(draws, np.float64), np.array(params, np.int32), np.stack(imgs), np.stack(gts)


def generate():
    _, registry = load_transforms()
    out = {}
    for group in (tc.OFF_CASES, tc.ON_CASES):
        for name, case in group.items():
            seqs, draws, params, img, gt = run_case(registry, case)
            for k, s in enumerate(seqs):
                out[f"{name}/seq{k}"] = s
            out[f"{name}/seed"] = np.int64(case["seed"])
            out[f"{name}/draws"], out[f"{name}/params"], out[f"{name}/img"], out[f"{name}/gt"] = draws, params, img, gt
            worst = 0.0
            for i, (k, t) in enumerate(tc.sample_sources(case)):
                r = tc.restate(seqs[k], t, *[int(v) for v in params[i]], draws[i, 5], case["pad"], case["crop"], case["K"])
                worst = max(worst, float(np.abs(r["img"] - img[i]).max()))
                assert np.array_equal(r["gt"], gt[i]), (name, i)
            print(f"[train_batch] {name:9s} map {case['map']} pad {case['pad']} crop {case['crop']} n {case['n']}: offsets r {sorted(set(params[:, 0].tolist()))} "
                  f"c {sorted(set(params[:, 1].tolist()))} flips {sorted(set(params[:, 2].tolist()))} rotate {params[:, 3].tolist()} "
                  f"gt non-zero {int((gt != 0).sum())}  restatement - pipeline {worst:.2e}")
    np.savez_compressed(tc.GOLDEN, **out)
    print(f"[train_batch] -> {tc.GOLDEN} ({os.path.getsize(tc.GOLDEN)} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    generate()
