"""Times sliding-window and flip-averaged inference (``HipSegmentor.inference``, ``peanut_pred_inference``) on one map at the sizes
the agent runs, 720 x 720 and 960 x 960, in three modes:

* ``whole_flip``   test_cfg whole, images [none, horizontal]
* ``slide``        crop 480 / stride 320 (4 windows at 720, 9 at 960), one image
* ``slide_flip``   both

Each against the only route there was before the call existed (``sequential``): one ``get_prediction_batch`` call per window and
image, and the pad-add / divide / flip / mean of the reference in torch on the device.  The two sides alternate in one process;
medians with [min, max] over ``--repeats`` windows of ``--calls`` calls, in milliseconds per call, timed with the host clock around
work that ends in a synchronise.  The gather and the combine launch are timed alone from device events
(``peanut_pred_infer_gather`` / ``_combine`` on buffers of the call's sizes).  Before anything is timed the two sides are compared.

    python -m tools.bench_infer [--out profiles/infer/infer.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CROP, STRIDE = (480, 480), (320, 320)
MODES = {"whole_flip": ("whole", (0, 1)), "slide": ("slide", (0,)), "slide_flip": ("slide", (0, 1))}
FLIP_DIMS = {1: (3,), 2: (2,)}


def spread(v):
    v = sorted(v)
    return {"median": round(statistics.median(v), 3), "min": round(v[0], 3), "max": round(v[-1], 3), "n": len(v)}


def sequential(model, x, mode, flips, wins):
    """The reference's loops on the device with one forward per window and image (encoder_decoder.py:155-201, 249-256, 273-291)."""
    B, _, H, W = x.shape
    out = None
    for f in flips:
        img = x.flip(FLIP_DIMS[f]) if f else x
        if mode == "slide":
            preds = x.new_zeros((B, model.model.cfg.num_classes, H, W))
            count = x.new_zeros((B, 1, H, W))
            for y1, x1, y2, x2 in wins:
                logit = model.get_prediction_batch(img[:, :, y1:y2, x1:x2].contiguous(), apply_sigmoid=False)
                preds += F.pad(logit, (x1, W - x2, y1, H - y2))
                count[:, :, y1:y2, x1:x2] += 1
            p = preds / count
        else:
            p = model.get_prediction_batch(img.contiguous(), apply_sigmoid=False)
        if f:
            p = p.flip(FLIP_DIMS[f])
        out = p if out is None else out + p
    if len(flips) > 1:
        out = out / len(flips)
    return torch.sigmoid(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "infer", "infer.jsonl"))
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sizes", default="720,960")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_infer measures on the GPU; no device is visible")
    from bench import synth_maps
    from peanut_amd import prediction as P
    from peanut_amd.weights import PredCfg, make_seeded_state_dict
    model = P.PEANUT_Prediction_Model(SimpleNamespace(sem_gpu_id=0), state_dict=make_seeded_state_dict(PredCfg(), 0), cfg=PredCfg())
    seg, stock = model.model, PredCfg()
    rows = []
    for size in (int(s) for s in a.sizes.split(",")):
        x = synth_maps(1, 14, size, "cuda", seed0=size)
        for name, (mode, flips) in MODES.items():
            cfg = PredCfg(test_mode=mode, crop_size=CROP if mode == "slide" else None, stride=STRIDE if mode == "slide" else None,
                          augs=tuple((bool(f), "horizontal") for f in flips))
            ys, xs, ch, cw = P.slide_windows(size, size, CROP, STRIDE) if mode == "slide" else ([0], [0], size, size)
            wins = [(y, x1, y + ch, x1 + cw) for y in ys for x1 in xs]

            def infer():
                seg.cfg = cfg                       # the handle is the same on both sides; only the descriptor's source differs
                try:
                    return seg.inference(x, apply_sigmoid=True)
                finally:
                    seg.cfg = stock

            def one_batch(n):
                for _ in range(n):
                    infer()

            def seq(n):
                for _ in range(n):
                    sequential(model, x, mode, flips, wins)
            diff = (infer() - sequential(model, x, mode, flips, wins)).abs().max().item()
            assert diff <= 5e-5, f"{name} at {size}: the two routes differ by {diff:.3e}"
            sides = {"one_batch": one_batch, "sequential": seq}
            for fn in sides.values():
                fn(2)
            t = {k: [] for k in sides}
            for _ in range(a.repeats):
                for k, fn in sides.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn(a.calls)
                    torch.cuda.synchronize()
                    t[k].append((time.perf_counter() - t0) / a.calls * 1e3)
            # the two glue launches alone, from device events
            d = P.infer_descriptor(mode, CROP if mode == "slide" else None, STRIDE if mode == "slide" else None, flips)
            staged = P.infer_gather(x, d)
            logits = torch.randn((staged.shape[0], 6, ch, cw), device="cuda")
            out = torch.empty((1, 6, size, size), device="cuda")
            glue = {"gather": [], "combine": []}
            for rep in range(a.repeats + 2):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                ev[0].record()
                P.infer_gather(x, d)
                ev[1].record()
                P.infer_combine(logits, d, 1, size, size, apply_sigmoid=True, out=out)
                ev[2].record()
                ev[2].synchronize()
                if rep >= 2:
                    glue["gather"].append(ev[0].elapsed_time(ev[1]))
                    glue["combine"].append(ev[1].elapsed_time(ev[2]))
            moved = (x.numel() + staged.numel() + logits.numel() + out.numel()) * 4
            row = {"section": "pred_inference", "mode": name, "size": size, "B": 1, "windows": len(wins), "augs": len(flips),
                   "maps_per_forward": staged.shape[0], "window": [ch, cw], "unit": "ms per call", **{k: spread(v) for k, v in t.items()},
                   "gather_ms": spread(glue["gather"]), "combine_ms": spread(glue["combine"]), "glue_bytes": moved,
                   "max_abs_between_routes": diff, "calls": a.calls, "gpu": torch.cuda.get_device_name(0)}
            row["sequential_over_one_batch"] = round(row["sequential"]["median"] / row["one_batch"]["median"], 3)
            row["below_by_more_than_both_spreads"] = bool(row["one_batch"]["max"] < row["sequential"]["min"])
            print(json.dumps(row), file=sys.stderr, flush=True)
            rows.append(row)
            del staged, logits, out
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    print(f"-> {a.out}")


if __name__ == "__main__":
    main()
