"""Times the visualisation frame at the deployed size: a 480 x 480 local map (14 planes) inside a 960 x 960 full map, a fp32
prediction normalised in double, float64 value and distance weights, a 480 x 640 RGB frame.

Rows for E = 1 / 4 / 8 / 16 episodes, the sides alternated in one process, medians with [min, max] over ``--repeats`` windows of
``--calls`` calls, in microseconds per call (one call renders E frames):

* ``device``           ``VisRenderer.render`` (E = 1) / ``render_batch``: three launches, timed to the end of the device work.
* ``device_prebuilt``  ``launch`` on argument structs made once by ``prepare``: the library call and the device work alone.
* ``host_prepare``     ``prepare`` alone: the checks, the ctypes structs and the arrow's vertices, E times; nothing is enqueued.
* ``device_readback``  the same and ``frame_host()``: the frames on the host through one pinned copy.
* ``host``             the reference's statements restated below (``host_frame``: NumPy, PIL's palette pass, matplotlib's colour map,
                       the nearest resize by indexing, scipy's dilation), run E times, with the plane downloads they need (the
                       semantic planes for the arg-max, obstacle, explored, the two planner maps' windows, the three fields).  The
                       arrow is left out on this side (cv2 draws it in the reference); the frames of the two sides are compared
                       outside the arrow's pixels before anything is timed.

    python -m tools.bench_vis [--out profiles/vis/vis.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    v = sorted(v)
    return {"median": round(statistics.median(v), 2), "min": round(v[0], 2), "max": round(v[-1], 2), "n": len(v)}


def _nearest_rows(n_dst, n_src):
    """Source index of every destination row / column under cv2's legacy INTER_NEAREST."""
    step = 1.0 / (float(n_dst) / float(n_src))
    return np.minimum(np.floor(np.arange(n_dst, dtype=np.float64) * step).astype(np.int64), n_src - 1)


def _purples_panel(field, cm, n):
    """A field as the reference colours it: min-max normalised in its own dtype, through matplotlib's 'Purples', upside down, BGR,
    resized to n x n; float64 [n, n, 3] in 0..255 (the caller's uint8 assignment truncates)."""
    with np.errstate(all="ignore"):
        lo, hi = np.min(field), np.max(field)
        bgr = cm((field - lo) / (hi - lo))[::-1, :, 2::-1] * 255
    pick = _nearest_rows(n, field.shape[0])
    return bgr[pick][:, pick]


def host_frame(item, background, palette, ncat, cm, disk4):
    """What the reference computes per step for one episode (the arg-max of agent_state.py:259-262 and the frame of
    agent_helper.py:507-592), restated with the host libraries it uses -- torch's arg-max and the plane downloads, NumPy, PIL's
    palette conversion, matplotlib's colour map, scipy's dilation -- from the device maps of ``item`` -> uint8 [600, 1415, 3]
    without the arrow."""
    from PIL import Image
    from scipy import ndimage as ndi
    r0, r1, c0, c1 = item["lmb"]
    planes = item["local_map"]
    cats = planes[4:].clone()
    cats[-1] = 1e-5
    # the downloads: the class map, two fp32 planes, the windows of the two planner maps, the goal map
    cls = cats.argmax(0).cpu().numpy() + 5
    obstacle = np.rint(planes[0].cpu().numpy()) == 1
    explored = np.rint(planes[1].cpu().numpy()) == 1
    bumped = item["collision_map"][r0:r1, c0:c1].cpu().numpy() == 1
    walked = item["visited_vis"][r0:r1, c0:c1].cpu().numpy() == 1
    near_goal = ndi.binary_dilation(item["goal"].cpu().numpy().astype(np.float64), structure=disk4)
    m = cls.shape[0]
    cls[bumped] = 14
    sr, sc = int(item["stg"][0]), int(item["stg"][1])
    if sr < m and sc < m:
        cls[sr, sc] = 15
    empty = cls == ncat + 4
    cls[empty] = 0
    cls[empty & explored] = 2
    cls[empty & obstacle] = 1
    cls[walked] = 3
    cls[near_goal] = 4
    # the palette pass, as PIL does it
    pal = Image.new("P", (m, m))
    pal.putpalette(palette)
    pal.putdata(cls.ravel().astype(np.uint8))
    colours = np.asarray(pal.convert("RGB"))[::-1, :, ::-1]
    pick = _nearest_rows(480, m)
    map_panel = colours[pick][:, pick]
    frame = background.copy()
    if item.get("rgb") is not None:
        frame[50:530, 15:655] = item["rgb"].cpu().numpy()[:, :, ::-1]
    frame[50:530, 670:1150] = map_panel
    if item.get("target_pred") is not None:
        pred = item["target_pred"].cpu().numpy()
        if item.get("target_bits", 32) == 64:
            pred = pred.astype(np.float64)
        blank = map_panel.astype(np.int64).sum(axis=2) == 765
        frame[50:530, 670:1150][blank] = _purples_panel(pred, cm, 480)[blank]
        frame[290:530, 1165:1405] = _purples_panel(item["value"].cpu().numpy(), cm, 240)
        frame[50:290, 1165:1405] = _purples_panel(item["dd_wt"].cpu().numpy(), cm, 240)
        frame[[49, 530], 1165:1405] = 100
        frame[49:531, 1405] = 100
    return frame


def host_tables():
    """(palette list, colour map, disk(4)) of the host route; needs matplotlib."""
    import matplotlib
    from peanut_amd import vis as pv
    L = np.arange(-4, 5)
    X, Y = np.meshgrid(L, L)
    return [int(v) for v in pv._PALETTE_RGB], matplotlib.colormaps["Purples"], (X ** 2 + Y ** 2) <= 16


def make_items(E, dev, m=480, full=960, ncat=10, seed=0):
    g = torch.Generator().manual_seed(seed)
    items = []
    for e in range(E):
        full_map = torch.rand((4 + ncat, full, full), generator=g) * 1.5
        full_map[4:, ::5] = 0.0
        full_map = full_map.to(dev)
        o = 200 + 8 * e
        lmb = [o, o + m, o + 16, o + 16 + m]
        goal = torch.zeros((m, m), dtype=torch.uint8)
        goal[100 + e, 200] = 1
        tp = torch.rand((m, m), generator=g)
        dd = torch.rand((m, m), generator=g, dtype=torch.float64)
        items.append(dict(local_map=full_map[:, lmb[0]:lmb[1], lmb[2]:lmb[3]],
                          collision_map=(torch.rand((full, full), generator=g) < 0.01).to(torch.uint8).to(dev),
                          visited_vis=(torch.rand((full, full), generator=g) < 0.01).to(torch.uint8).to(dev), lmb=lmb, goal=goal.to(dev),
                          stg=(240.0 + e, 200.0), pose_pred=np.array([(lmb[2] + 240) * 0.05, (lmb[0] + 240) * 0.05, 30.0 * e, *lmb], np.float64),
                          goal_name="chair", rgb=(torch.rand((480, 640, 3), generator=g) * 256).to(torch.uint8).to(dev),
                          target_pred=tp.to(dev), value=(tp.double() * dd).to(dev), dd_wt=dd.to(dev), target_bits=64))
    return items


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vis", "vis.jsonl"))
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batches", default="1,4,8,16")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_vis measures on the GPU; no device is visible")
    from peanut_amd import vis as pv
    dev = torch.device("cuda:0")
    ncat = 10
    r = pv.VisRenderer(SimpleNamespace(num_sem_categories=ncat, map_resolution=5), dev)
    palette, cm, disk4 = host_tables()
    background = pv.init_vis_image("chair", None)
    rows = []
    for E in (int(b) for b in a.batches.split(",")):
        items = make_items(E, dev)
        r.render_batch(items)
        got = r.frame_host()
        for e, it in enumerate(items):                  # the two sides agree outside the arrow
            want = host_frame(it, background, palette, ncat, cm, disk4)
            pts = pv.contour_points(pv.arrow_pos(it["pose_pred"], 480, 5))
            x0, x1, y0, y1 = pts[:, 0].min(), pts[:, 0].max(), pts[:, 1].min(), pts[:, 1].max()
            diff = (got[e] != want).any(axis=2)
            diff[y0:y1 + 1, x0:x1 + 1] = False
            assert not diff.any(), f"E = {E}, episode {e}: {int(diff.sum())} pixels differ between the device and the host route"

        def device(n):
            for _ in range(n):
                r.render_batch(items)

        prepared = r.prepare(items)

        def device_prebuilt(n):                         # the library call alone: checks, structs and arrow vertices made once
            for _ in range(n):
                r.launch(prepared)

        def host_prepare(n):                            # the host half alone; nothing is enqueued
            for _ in range(n):
                r.prepare(items)

        def device_readback(n):
            for _ in range(n):
                r.render_batch(items)
                r.frame_host()

        def host(n):
            for _ in range(n):
                for it in items:
                    host_frame(it, background, palette, ncat, cm, disk4)
        sides = {"device": (device, a.calls), "device_prebuilt": (device_prebuilt, a.calls), "host_prepare": (host_prepare, a.calls),
                 "device_readback": (device_readback, a.calls), "host": (host, max(1, a.calls // 10))}
        for fn, _ in sides.values():
            fn(2)
        t = {k: [] for k in sides}
        for _ in range(a.repeats):
            for k, (fn, n) in sides.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(n)
                torch.cuda.synchronize()
                t[k].append((time.perf_counter() - t0) / n * 1e6)
        row = {"section": "vis_render", "E": E, "m": 480, "ncat": ncat, "unit": "us per call (E frames)", **{k: spread(v) for k, v in t.items()},
               "calls": {k: n for k, (_, n) in sides.items()}, "gpu": torch.cuda.get_device_name(0)}
        row["host_over_device_readback"] = round(row["host"]["median"] / row["device_readback"]["median"], 1)
        print(json.dumps(row), file=sys.stderr, flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    print(f"-> {a.out}")


if __name__ == "__main__":
    main()
