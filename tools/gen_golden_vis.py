"""Writes tests/golden/vis_golden.npz: what the reference's OWN ``Agent_Helper._visualize`` (nav/agent/agent_helper.py:496-621),
``init_vis_image`` and ``get_contour_points`` (nav/agent/utils/visualization.py:5-16, 27-83) give on the cases of tests/vis_cases.py.

The reference's modules are imported at run time, unmodified, under the stand-ins of tools/gen_golden_stg.load_reference plus a
``cv2`` stand-in: ``resize`` is the stated legacy INTER_NEAREST rule (``min(int(floor(dst * ifx)), n - 1)``, ``ifx = 1.0 / (dst_n /
src_n)``; at the sizes stored here -- m = 480, 240, 96, 8, 1 -- the ratios 480 / m and 240 / m are 1, 2, 5, 60, 480 and 0.5, 1, 2.5, 30,
240, exact in binary, so every rule that takes the nearest lower source cell agrees with it), ``putText`` /
``getTextSize`` are inert (no titles), ``drawContours`` and ``imwrite`` record their arguments.  ``_visualize`` is called unbound on
a stand-in object with the fields it reads.  PIL and matplotlib are the real ones.  So the file pins: the index map, the whole frame
WITHOUT the arrow, the arrow's vertices and colour, the file name.  It does not pin the arrow's fill, the titles or the JPEG bytes.

It also checks, and prints, the two tables peanut_amd/vis.py carries as constants (the palette bytes, the 257 x 3 'Purples' table),
this package's ``init_vis_image`` / ``contour_points`` and the restatement of tests/vis_cases.py against the reference.

Needs the reference checkout (it does not travel with the tests; the .npz does).

    python -m tools.gen_golden_vis
"""
from __future__ import annotations

import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import vis_cases as vc                              # noqa: E402
from peanut_amd import vis as pv                    # noqa: E402
from tools.gen_golden_stg import load_reference     # noqa: E402


def purples_table():
    """``(cm(i)[[2, 1, 0]] * 255).astype(uint8)`` for i = 0..255 and the "bad" colour -> uint8 [257, 3]."""
    import matplotlib
    cm = matplotlib.colormaps["Purples"]
    rows = [(np.array(cm(i))[[2, 1, 0]] * 255).astype(np.uint8) for i in range(256)]
    rows.append((np.array(cm(np.array([np.nan]))[0])[[2, 1, 0]] * 255).astype(np.uint8))
    return np.array(rows, np.uint8)


def cv2_stand_in(record):
    cv2 = types.ModuleType("cv2")
    cv2.INTER_NEAREST, cv2.FONT_HERSHEY_DUPLEX, cv2.LINE_AA, cv2.IMWRITE_JPEG_QUALITY = 0, 2, 16, 1

    def resize(src, dsize, interpolation=None):
        assert interpolation == cv2.INTER_NEAREST
        rows, cols = vc.nearest_index(dsize[1], src.shape[0]), vc.nearest_index(dsize[0], src.shape[1])
        return np.ascontiguousarray(np.asarray(src)[rows][:, cols])

    cv2.resize = resize
    cv2.getTextSize = lambda *a, **k: ((0, 0), 0)
    cv2.putText = lambda img, *a, **k: img
    cv2.drawContours = lambda img, contours, idx, color, thickness: record.append(("contours", np.array(contours[idx]), tuple(color), thickness))
    cv2.imwrite = lambda fn, img, params=None: record.append(("imwrite", fn, np.array(img), params))
    cv2.imshow = lambda *a, **k: None
    cv2.waitKey = lambda *a, **k: None
    return cv2


def run_reference(ah, case, record, dump):
    """The reference's ``_visualize`` on a case -> (index map, frame without the arrow, vertices, colour, file name)."""
    import torch
    m = case["m"]
    gx1, gx2, gy1, gy2 = case["lmb"]
    lm = case["full_map"][:, gx1:gx2, gy1:gy2]
    vlm = torch.clone(torch.from_numpy(np.ascontiguousarray(lm[4:])))          # agent_state.py:259-262, as written
    vlm[-1] = 1e-5
    sem = vlm.argmax(0).cpu().numpy()
    assert np.array_equal(sem, vc.sem_argmax(lm)), f"{case['name']}: torch's arg-max is not the first maximum"
    x, y, o = case["pose"]
    inputs = dict(obstacle=np.ascontiguousarray(lm[0]), exp_pred=np.ascontiguousarray(lm[1]),
                  pose_pred=np.array([x, y, o, gx1, gx2, gy1, gy2], np.float64), goal=case["goal"].astype(np.float64), sem_map_pred=sem)
    args = types.SimpleNamespace(dump_location=dump, exp_name="exp", num_sem_categories=case["ncat"], map_resolution=vc.RES, visualize=2)
    white = np.full((480, 640, 3), 255, np.uint8)                             # rgb None: the background's own white
    me = types.SimpleNamespace(args=args, rank=case["rank"], episode_no=case["episode_no"], timestep=case["timestep"],
                               goal_name=case["goal_name"], legend=vc.legend(), collision_map=case["collision"].astype(np.float64),
                               visited_vis=case["visited"].astype(np.float64), stg=case["stg"], local_w=m, local_h=m,
                               rgb_vis=white if case["rgb"] is None else case["rgb"][:, :, ::-1],
                               agent_states=types.SimpleNamespace(target_pred=case["target_pred"], value=case["value"], dd_wt=case["dd_wt"]))
    del record[:]
    with np.errstate(all="ignore"):
        ah.Agent_Helper._visualize(me, inputs)
    (_, pts, colour, thickness), (_, fn, img, params) = record
    assert thickness == -1 and params == [1, 100] and np.array_equal(img, me.vis_image)
    assert fn.startswith(dump)
    return inputs["sem_map_pred"], img, pts, colour, "D" + fn[len(dump):]


def generate():
    record = []
    sys.modules["cv2"] = cv2_stand_in(record)
    ah, _ = load_reference()
    import agent.utils.visualization as vu          # type: ignore
    import constants                                # type: ignore
    # the tables peanut_amd/vis.py carries
    pal = [int(v * 255.) for v in constants.color_palette]
    assert tuple(pal) == pv._PALETTE_RGB, f"palette bytes:\n{pal}"
    table = purples_table()
    assert np.array_equal(table, pv.purples_bgr()), f"'Purples' table:\n{table.tobytes().hex()}"
    assert pv.arrow_colour() == (int(constants.color_palette[11] * 255), int(constants.color_palette[10] * 255), int(constants.color_palette[9] * 255))
    for name in ("chair", "tv_monitor"):
        assert np.array_equal(vu.init_vis_image(name, vc.legend()), pv.init_vis_image(name, vc.legend())), "init_vis_image"
    out = {}
    with tempfile.TemporaryDirectory() as dump:
        for c in vc.golden_cases():
            sem, frame, pts, colour, fn = run_reference(ah, c, record, dump)
            assert sem.min() >= 0 and sem.max() <= 255
            assert np.array_equal(sem, vc.index_map(c)), f"{c['name']}: the restated index map differs"
            mine = vc.restate(c, pv.init_vis_image(c["goal_name"], vc.legend()), pv.palette_lut(), pv.purples_bgr())
            assert np.array_equal(frame, mine), f"{c['name']}: the restated frame differs in {int((frame != mine).any(axis=2).sum())} pixels"
            x, y, o = c["pose"]
            pose = np.array([x, y, o, *c["lmb"]], np.float64)
            assert np.array_equal(pts, pv.contour_points(pv.arrow_pos(pose, c["m"], vc.RES))), f"{c['name']}: contour points"
            assert tuple(colour) == pv.arrow_colour()
            args = types.SimpleNamespace(dump_location="D", exp_name="exp")
            assert pv.frame_path(args, c["rank"], c["episode_no"], c["timestep"])[1] == fn, fn
            k = c["name"]
            out[f"{k}/index"] = sem.astype(np.uint8)
            out[f"{k}/frame"] = frame
            out[f"{k}/arrow"] = np.asarray(pts, np.int64)
            out[f"{k}/colour"] = np.array(colour, np.int64)
            out[f"{k}/fname"] = np.frombuffer(fn.encode(), np.uint8)
            print(f"[vis] {k:12s} m {c['m']:3d} ncat {c['ncat']:2d} index values {sorted(set(sem.ravel().tolist()))} arrow {pts.tolist()}")
    np.savez_compressed(vc.GOLDEN, **out)
    print(f"[vis] -> {vc.GOLDEN} ({os.path.getsize(vc.GOLDEN)} bytes)")


if __name__ == "__main__":
    generate()
