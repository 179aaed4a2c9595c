"""Writes tests/golden/infer_golden.npz: what the reference's OWN ``EncoderDecoder`` returns under
``test_cfg.mode='slide'`` and under flipped test-time augmentations -- ``slide_inference`` (encoder_decoder.py:155-201), the flip branch
of ``inference`` (:249-256), ``aug_test`` (:273-291), reached through ``forward_test`` (segmentors/base.py:62-110) -- on the cases of
tests/infer_cases.py.

The model is built by the committed import recipe (oracle/ref_import.py, the reference's model files unmodified) with the seeded state
dict; ``model.test_cfg`` is then set to the case's crop and stride and the model is called as nav/agent/prediction.py:135-136 calls
it, with one image and one meta list per augmentation: the image flipped as the pipeline's RandomFlip flips it (``np.flip`` of the
whole image), the meta saying so.  The file holds results only: ``<case>/slide/<aug list>`` (float32 [B, K, H, W]) for every case
and aug list, and ``<case>/distance/<aug list>``, the max-abs distance of that result to the reference's whole_inference of the
unflipped image (what the agent gets today).  The tool prints the distances; tests/test_infer_cpu.py re-checks them from the file
against the oracle's whole result.

Needs the reference checkout (it does not travel with the tests; the .npz does).

    python -m tools.gen_golden_infer
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import infer_cases as ic                                        # noqa: E402
from oracle import ref_import                                    # noqa: E402
from peanut_amd.weights import PredCfg, make_seeded_state_dict   # noqa: E402


def reference_model():
    m = ref_import.build_reference_model(in_channels=PredCfg().in_channels)
    m.load_state_dict(make_seeded_state_dict(PredCfg(), 0, with_aux=True), strict=True)
    return m


def run_reference(model, x, flips, test_cfg):
    """``model(return_loss=False, rescale=True, img=[...], img_metas=[[...], ...])`` -> float32 [B, K, H, W]."""
    n, c, h, w = x.shape
    model.test_cfg = ref_import.to_cfg(test_cfg)
    imgs, metas = [], []
    for f in flips:
        meta = dict(ori_shape=(h, w, c), img_shape=(h, w, c), pad_shape=(h, w, c), scale_factor=1.0, flip=bool(f))
        if f:
            meta["flip_direction"] = ic.FLIP_NAMES[f]
        imgs.append(ic.flip(x, f).contiguous())
        metas.append([meta] * n)
    with torch.no_grad():
        return np.stack(model(return_loss=False, rescale=True, img=imgs, img_metas=metas)).astype(np.float32)


def generate():
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    model = reference_model()
    out = {}
    for case, c in ic.CASES.items():
        x = ic.inputs(case)
        whole = run_reference(model, x, (0,), dict(mode="whole"))
        cnt = ic.count_matrix(c["H"], c["W"], c["crop"], c["stride"])
        assert cnt.min() >= 1
        if case in ic.COUNTS:
            assert set(np.unique(cnt).tolist()) == ic.COUNTS[case], (case, np.unique(cnt))
        for name, flips in ic.AUG_LISTS.items():
            y = run_reference(model, x, flips, dict(mode="slide", crop_size=c["crop"], stride=c["stride"]))
            assert y.shape == whole.shape and np.isfinite(y).all()
            out[ic.key(case, name)] = y
            out[ic.key(case, name, "distance")] = np.float32(np.abs(y - whole).max())
            print(f"[infer] {case} {c['H']:2d}x{c['W']:2d} B {c['B']} crop {c['crop']} stride {c['stride']} counts {sorted(set(cnt.ravel().tolist()))} "
                  f"{name:9s} max |logit| {np.abs(y).max():.2f}  distance to whole/none {np.abs(y - whole).max():.3f}")
    np.savez_compressed(ic.GOLDEN, **out)
    print(f"[infer] -> {ic.GOLDEN} ({os.path.getsize(ic.GOLDEN)} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    generate()
