#!/usr/bin/env python3
"""Score a prediction checkpoint on stored map sequences with the loss it was trained on (the reference's `my_loss`,
prediction/train_prediction_model.py:173-184, on the samples `SemMapDataset.load_annotations` lists: per file t_idx 0..9, files
sorted by name).  The sequences go up as uint8, inputs, forward and loss stay on the device (peanut_amd.mapio.evaluate).

    python tools/eval_maps.py data/saved_maps/val_80 --weights nav/pred_model_wts.pth [--cfg nav/pred_model_cfg.py]
                              [--precision fp32|bf16x6|fp16x3|bf16x3] [--window 720] [--t-indices 0-9] [--batch 10]
                              [--augment SEED [--pad 1200 --crop 960]]

prints one JSON line: loss (mean over all cells, reduction='mean', weight 1.0), loss_per_channel, n_maps, maps_per_s.
`--augment SEED` scores under the training augmentation instead (the reference's train_pipeline: pad, random crop, flip 0.5, rotation
+-180 degrees, drawn from SEED): how robust the checkpoint is to the shifts and rotations it was trained with.
`--seeded SEED` replaces the checkpoint by the seeded synthetic weights (a dry run of the path, not a score)."""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _t_indices(text):
    out = []
    for part in text.split(","):
        if "-" in part:
            lo, hi = part.split("-")
            out += list(range(int(lo), int(hi) + 1))
        else:
            out.append(int(part))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("paths", nargs="+", help=".npz files or directories of them")
    ap.add_argument("--weights", default=None, help="mmcv checkpoint of the prediction model")
    ap.add_argument("--cfg", default=None, help="mmcv-style model config (default: the reference's pred_model_cfg.py values)")
    ap.add_argument("--seeded", type=int, default=None, help="seeded synthetic weights instead of a checkpoint")
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16x6", "fp16x3", "bf16x3"])
    ap.add_argument("--window", type=int, default=None, help="centre crop fed to the model (default: the whole map)")
    ap.add_argument("--t-indices", default="0-9")
    ap.add_argument("--batch", type=int, default=None, help="samples per forward (default: all samples of a file)")
    ap.add_argument("--augment", type=int, default=None, metavar="SEED", help="score under the training augmentation drawn from SEED")
    ap.add_argument("--pad", type=int, default=1200, help="with --augment: the pad size (nav/pred_model_cfg.py:50)")
    ap.add_argument("--crop", type=int, default=960, help="with --augment: the crop size (nav/pred_model_cfg.py:51)")
    ap.add_argument("--gpu", type=int, default=0)
    a = ap.parse_args()
    if (a.weights is None) == (a.seeded is None):
        ap.error("give either --weights or --seeded")
    import torch

    from peanut_amd import mapio
    from peanut_amd.prediction import PEANUT_Prediction_Model
    from peanut_amd.weights import PredCfg, make_seeded_state_dict, pred_cfg_from_file
    cfg = pred_cfg_from_file(a.cfg) if a.cfg else PredCfg()
    args = SimpleNamespace(sem_gpu_id=a.gpu, pred_model_wts=a.weights, pred_model_cfg=a.cfg)
    sd = make_seeded_state_dict(cfg, a.seeded) if a.seeded is not None else None
    model = PEANUT_Prediction_Model(args, state_dict=sd, cfg=cfg, precision=a.precision)
    files = mapio.dataset_files(a.paths)
    if not files:
        sys.exit("no .npz files under " + " ".join(a.paths))
    t0 = time.perf_counter()
    augment = mapio.TrainAugment(a.pad, a.crop, seed=a.augment) if a.augment is not None else None
    res = mapio.evaluate(model, files, t_indices=_t_indices(a.t_indices), window=a.window, batch=a.batch, augment=augment)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    res.update(precision=a.precision, files=len(files), window=a.window, augment=a.augment, seconds=round(dt, 3), maps_per_s=round(res["n_maps"] / dt, 2))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
