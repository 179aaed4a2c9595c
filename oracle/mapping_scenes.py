"""ORACLE support (test infrastructure): seeded synthetic observation sequences for the
map-projection path -- analytic floor / wall / box depth images in the units
``_preprocess_depth`` produces (nav/agent/agent_helper.py:197-217: cm = 50 + d*450, invalid or
too-far pixels = 45050), plus rectangular semantic masks.  Shapes follow nav/arguments.py
(120x160 frames, 10 semantic channels)."""
from __future__ import annotations

import math
from typing import Dict, List

import numpy as np

FAR_CM = 50.0 + 100.0 * 450.0      # what invalid / >0.99 depth turns into


def _floor_depth(h, w, hfov, cam_h_cm, floor_h_cm):
    xc, zc = (w - 1.0) / 2.0, (h - 1.0) / 2.0
    f = (w / 2.0) / math.tan(math.radians(hfov / 2.0))
    gz = np.arange(h - 1, -1, -1, dtype=np.float64)[:, None].repeat(w, 1)   # flipped row index
    below = zc - gz                                                          # > 0 below the horizon
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.where(below > 0, (cam_h_cm - floor_h_cm) * f / below, np.inf)
    return d


def make_sequence(seed: int = 0, n_frames: int = 8, h: int = 120, w: int = 160, ncat: int = 10,
                  hfov: float = 79.0, cam_h_cm: float = 88.0) -> List[Dict[str, np.ndarray]]:
    """Frames: dict(depth f32 [h,w] in cm (quantised to 1/4 cm so fixtures compress), sem u8
    [ncat,h,w], pose f32 [3] = (dx m, dy m, dtheta rad)).  Frame 3 looks at a raised floor (30 cm,
    triggers the low-stairs branch mapping.py:94), frame 5 has a far/invalid band (points outside
    the grid) and overlapping instance masks (value 2)."""
    rng = np.random.RandomState(seed)
    frames = []
    for i in range(n_frames):
        floor_h = 30.0 if i == 3 else 0.0
        d = _floor_depth(h, w, hfov, cam_h_cm, floor_h)
        wall = rng.uniform(180.0, 420.0)
        # a slanted wall: depth varies linearly across columns
        slope = rng.uniform(-0.6, 0.6)
        wall_d = wall + slope * (np.arange(w)[None, :] - w / 2.0)
        d = np.minimum(d, wall_d)
        # two boxes closer than the wall
        for _ in range(2):
            r0, c0 = rng.randint(20, h - 50), rng.randint(5, w - 45)
            hh, ww = rng.randint(15, 45), rng.randint(15, 40)
            bd = rng.uniform(70.0, wall * 0.8)
            d[r0:r0 + hh, c0:c0 + ww] = np.minimum(d[r0:r0 + hh, c0:c0 + ww], bd)
        d = d + rng.uniform(-1.0, 1.0, size=d.shape)              # sensor noise
        d = np.clip(d, 50.0, 495.5)
        if i == 5:
            d[:, 120:] = FAR_CM                                    # invalid band -> outside the grid
        d = np.round(d * 4.0) / 4.0
        sem = np.zeros((ncat, h, w), np.uint8)
        for _ in range(3):
            k = rng.randint(0, ncat - 1)
            r0, c0 = rng.randint(10, h - 40), rng.randint(5, w - 40)
            sem[k, r0:r0 + rng.randint(10, 35), c0:c0 + rng.randint(10, 35)] += 1
        if i in (3, 5):
            sem[4, 60:100, 40:90] += 1                             # 'toilet' row (feat[0,5]) region
        if i == 5:
            sem[1, 30:60, 30:70] += 1
            sem[1, 40:70, 50:90] += 1                              # overlapping instances -> value 2
        pose = np.array([rng.uniform(0.0, 0.3), rng.uniform(-0.05, 0.05),
                         rng.choice([0.0, math.radians(30.0), -math.radians(30.0), rng.uniform(-0.2, 0.2)])],
                        np.float32)
        frames.append(dict(depth=d.astype(np.float32), sem=sem, pose=pose))
    return frames


def frame_to_obs(frame, ncat: int = 10) -> np.ndarray:
    """[4+ncat,h,w] float32 observation: RGB (unused by the mapping) zero, ch 3 depth, ch 4.. sem."""
    h, w = frame["depth"].shape
    obs = np.zeros((4 + ncat, h, w), np.float32)
    obs[3] = frame["depth"]
    obs[4:] = frame["sem"].astype(np.float32)
    return obs


# ---- edge scenes: the inputs make_sequence never produces (stairs rule at its thresholds, dense cells, grid limits,
#      heading wrap, starts at the border of the local map).  Small, deterministic, same frame format. ----
OUT_CM = 60000.0      # a depth that puts z outside (-1, 1) on EVERY row of the 120-row frame (FAR_CM leaves row 59 in range)
CENTRE = (12.0, 12.0, 0.0)      # agent_state.py init_map_and_pose: the middle of the 24 m local map, heading 0


def _camera(h, w, hfov):
    return (w - 1.0) / 2.0, (h - 1.0) / 2.0, (w / 2.0) / math.tan(math.radians(hfov / 2.0))


def _frame(depth, sem=None, pose=(0.0, 0.0, 0.0), ncat=10):
    h, w = depth.shape
    return dict(depth=np.asarray(depth, np.float32), sem=np.zeros((ncat, h, w), np.uint8) if sem is None else sem,
                pose=np.asarray(pose, np.float32))


def height_frame(heights, hfov: float = 79.0, cam_h_cm: float = 88.0) -> np.ndarray:
    """Depth image [h,w] (float32, NOT quantised) that puts pixel (r, c) at height ``heights[r, c]`` cm above the agent's
    floor: z = cam_h - (r - zc) d / f, so d = (cam_h - Z) f / (r - zc); my_z of mapping.py:91 is then Z / 100 up to rounding.
    NaN = pixel not used: it gets OUT_CM and never enters the stairs statistics or the grid."""
    heights = np.asarray(heights, np.float64)
    h, w = heights.shape
    _, zc, f = _camera(h, w, hfov)
    rows = np.arange(h, dtype=np.float64)[:, None] - zc
    used = ~np.isnan(heights)
    d = np.where(used, (cam_h_cm - np.where(used, heights, 0.0)) * f / rows, OUT_CM)
    assert np.all(d[used] > 0.0), "a height above the camera needs a row above the horizon, and the other way round"
    return d.astype(np.float32)


def _block_sem(h, w, ncat):
    """Rectangular masks (they compress): channels 2 and 5 are the all-height categories, 4 ('toilet') stays empty."""
    sem = np.zeros((ncat, h, w), np.uint8)
    sem[0, 76:, :] = 1
    sem[2, :, 60:100] = 1
    sem[5, 90:, :] = 1
    sem[7, 80:110, 50:80] = 2
    return sem


def _stairs_pixels(h=120, w=160):
    """The pixels the stairs frames fill, in a fixed order: rows 119..76, columns 40..119.  For every height in [5, 80] cm
    they land inside the 100 x 100 window (depth 13 .. 490 cm, |x| < 200 cm)."""
    return [(r, c) for r in range(h - 1, 75, -1) for c in range(40, 120)]


def _sharp_pixels(Z, k, h=120, w=160, hfov=79.0, cam_h_cm=88.0, res=5.0, shift_x=250.0):
    """The k stairs pixels whose point at height Z lies closest to a cell corner in x and y, so that a single point still
    rounds to 1 in one voxel (a lone point elsewhere spreads over 8 voxels and rounds away)."""
    xc, zc, f = _camera(h, w, hfov)
    scored = []
    for r, c in _stairs_pixels(h, w):
        d = (cam_h_cm - Z) * f / (r - zc)
        px, py = ((c - xc) * d / f + shift_x) / res, d / res
        fx, fy = px - math.floor(px), py - math.floor(py)
        scored.append((-max(fx, 1 - fx) * max(fy, 1 - fy), r, c))
    return [(r, c) for _, r, c in sorted(scored)[:k]]


def stairs_frame(groups, toilet: int = 0, sharp: bool = False, h=120, w=160, ncat=10):
    """``groups`` = [(height cm, count), ...] laid out over _stairs_pixels() in order (``sharp``: one pixel per group, chosen
    by _sharp_pixels); the first ``toilet`` pixels also carry sem channel 4 (feature row 5)."""
    heights = np.full((h, w), np.nan)
    if sharp:
        taken, pix = set(), []
        for Z, cnt in groups:
            assert cnt == 1
            p = next(q for q in _sharp_pixels(Z, 1 + len(taken), h, w) if q not in taken)
            taken.add(p)
            pix.append(p)
    else:
        pix = _stairs_pixels(h, w)
    i = 0
    for Z, cnt in groups:
        for r, c in pix[i:i + cnt]:
            heights[r, c] = Z
        i += cnt
    assert i <= len(pix)
    sem = _block_sem(h, w, ncat)
    for r, c in pix[:toilet]:
        sem[4, r, c] = 1
    return _frame(height_frame(heights), sem)


def stairs_pairs():
    """Pairs of frames on opposite sides of mapping.py:94, each with its design: n = #points with z in (-1, 1), le = #those
    with my_z <= 0.2, mid = #those in (0.2, 0.7), and whether the branch is taken.  With n = 1000 the quantile's rank is
    0.03 * 999 = 29.97: k_lo = 29, k_hi = 30, weight 0.97 -- interpolated only when le = 30."""
    lo, mid, hi = 5.0, 45.0, 80.0        # my_z 0.05 (at or below 0.2), 0.45 (in the band, removed), 0.80 (kept, agent height)
    P = []

    def pair(name, ga, gb, n, le, midc, taken, **kw):
        kwa, kwb = ({k: v[0] for k, v in kw.items()}, {k: v[1] for k, v in kw.items()})
        P.append(dict(name=name, a=stairs_frame(ga, **kwa), b=stairs_frame(gb, **kwb), n=n, le=le, mid=midc, taken=taken))
    # le = k_lo + 1: the quantile is max_le + 0.97 (min_gt - max_le) with max_le = 0.10: 0.2067 against 0.1975
    pair("interp", [(lo, 29), (10.0, 1), (21.0, 1), (mid, 599), (hi, 370)], [(lo, 29), (10.0, 1), (20.05, 1), (mid, 599), (hi, 370)],
         (1000, 1000), (30, 30), (600, 600), (True, False))
    # the two sides that need no interpolation: le = k_lo, le = k_hi + 1
    pair("le_sides", [(lo, 29), (mid, 601), (hi, 370)], [(lo, 31), (mid, 599), (hi, 370)],
         (1000, 1000), (29, 31), (601, 599), (True, False))
    # mid > 0.2 n at equality
    pair("mid_200", [(mid, 200), (hi, 1), (hi, 799)], [(mid, 200), (mid, 1), (hi, 799)],
         (1000, 1000), (0, 0), (200, 201), (False, True))
    # one point on either side.  (In b the point lies below the agent-height band, as every point at or below 0.2 does:
    # a wrong decision there shows in the explored channel of the map, not in fp_map_pred.)
    pair("n1", [(mid, 1)], [(15.0, 1)], (1, 1), (0, 1), (1, 0), (True, False), sharp=(True, True))
    # n = 2: rank 0.03, always interpolated when le = 1: 0.199 + 0.03 (0.65 - 0.199) = 0.2125 against 0.15 + 0.03 * 0.5 = 0.165
    pair("n2", [(19.9, 1), (65.0, 1)], [(15.0, 1), (65.0, 1)], (2, 2), (1, 1), (1, 1), (True, False), sharp=(True, True))
    # n = 101: the rank 0.03 * 100 is integral (k_lo = k_hi = 3)
    pair("n101", [(lo, 3), (mid, 60), (hi, 38)], [(lo, 4), (mid, 59), (hi, 38)], (101, 101), (3, 4), (60, 59), (True, False))
    # 'toilet' pixels inside the removed band survive the branch
    pair("toilet", [(mid, 200), (mid, 1), (hi, 799)], [(mid, 200), (hi, 1), (hi, 799)],
         (1000, 1000), (0, 0), (201, 200), (True, False), toilet=(100, 0))
    return P


def stairs_empty_frame():
    """n = 0: every z out of (-1, 1).  No decision can show in any output (no point is inside the grid); the frame is there
    for the division-free early exit."""
    return stairs_frame([])


def _random_sem(seed, h, w, ncat, channels=(0, 2, 4), sparse=()):
    """Random 0/1/2 values on ``channels``; ``sparse`` = ((channel, p), ...) are non-zero on a fraction p of the pixels only."""
    rng = np.random.RandomState(seed)
    sem = np.zeros((ncat, h, w), np.uint8)
    for k in channels:
        sem[k] = rng.randint(0, 3, size=(h, w))
    for k, p in sparse:
        sem[k] = rng.randint(1, 3, size=(h, w)) * (rng.uniform(size=(h, w)) < p)
    return sem


def dense_frame(depth_cm: float, seed: int, h=120, w=160, ncat=10):
    """A wall at constant depth with random 0/1/2 semantics: 55 cm (just above the sensor's minimum range) gives 300 floor
    cells with up to 81 points, 10 cm (not a value the depth preprocessing produces) 12 cells with up to 2352.  With a
    thousand points per map cell the dense channels saturate; the sparse ones (1, 5, 7, 8; channel 5 is an all-height
    category) stay below the category threshold, so their voxel values show in the map."""
    return _frame(np.full((h, w), depth_cm),
                  _random_sem(seed, h, w, ncat, sparse=((1, 0.003), (5, 0.001), (7, 0.0005), (8, 0.0002))))


ORDER_BIG_CM = 4.1088032722473145      # see order_frame
ORDER_VOXEL = (51, 1, 25)              # (x, y, z) of the voxel whose value depends on the order


def order_frame(h=120, w=160, ncat=10):
    """One floor cell, (50, 0, 25), whose sum for voxel (51, 1, 25) depends on the ORDER of its 3841 points in a way that
    survives the rounding and shows in the map.  3840 points at 0.0015 cm (columns 80..111) each give that voxel a weight
    below 1.2e-8, 2.33e-5 in all; the last pixel of the frame, at ORDER_BIG_CM, gives 0.49998277.  In point order the small
    ones come first: 2.33e-5 + 0.49998277 > 0.5 rounds to 1.  Any order that puts the large one before more than a quarter
    of the small ones loses them one by one (each is below half an ulp of 0.4999...): the sum stays at or below 0.5 and
    rounds to 0.  The voxel is the only one of its column that is not 0: explored area and the two all-height categories of
    window cell (1, 51) are 1, 0.2, 0.2 or 0.  (Depths no sensor gives; the ABI accepts them.)"""
    d = np.full((h, w), FAR_CM)
    d[:, 80:112] = 0.0015
    d[h - 1, w - 1] = ORDER_BIG_CM
    sem = np.zeros((ncat, h, w), np.uint8)
    sem[2] = 1
    sem[5] = 1
    sem[7] = 1
    return _frame(d, sem)


def far_frame(h=120, w=160):
    return _frame(np.full((h, w), FAR_CM))


def dense_sequence():
    """dense -> all-far -> the same cells again -> the densest cells -> an ordinary frame, all at the centre without motion:
    a per-cell table that is not re-armed shows in the frames after the empty one."""
    last = make_sequence(52, 1)[0]
    last["pose"] = np.zeros(3, np.float32)
    return [dense_frame(55.0, 1), far_frame(), dense_frame(55.0, 2), dense_frame(10.0, 3), last]


def limit_frames(h=120, w=160, ncat=10, hfov=79.0):
    """Three frames whose points cross the limits of the (100, 100, 80) voxel grid, one dimension each:
    z -- a floor sloping from 55 to 25 cm BELOW the agent's (pz from -3 to 3) and a ceiling from 345 to 370 cm (pz 77 .. 82);
    y -- depths 494 .. 501 cm in 1/4 cm steps (py 98.8 .. 100.2, 495 and 500 exactly on a cell), a few pixels at -4 .. 6 cm
         (py -0.8 .. 1.2), and a band of exact multiples of the cell size (weights exactly 1 and 0);
    x -- depths 296 .. 312.75 cm at the four outermost columns of either side (px 1.5 .. -1.2 and 98.5 .. 101.2)."""
    heights = np.full((h, w), np.nan)
    cols = np.arange(w)
    heights[70:119, :] = (-55.0 + 30.0 * cols / (w - 1))[None, :]
    heights[0:50, :] = (345.0 + 25.0 * cols / (w - 1))[None, :]
    fz = _frame(height_frame(heights, hfov), _random_sem(4, h, w, ncat, (1, 2, 5)))
    dy = np.full((h, w), FAR_CM)
    dy[40:81, :] = (494.0 + 0.25 * (cols % 29))[None, :]
    dy[20:30, 60:101] = (-4.0 + 0.25 * np.arange(41))[None, :]
    dy[90:110, :] = (5.0 * (10 + (cols // 2) % 85))[None, :]
    fy = _frame(dy, _random_sem(5, h, w, ncat, (1, 2, 5)))
    dx = np.full((h, w), FAR_CM)
    ramp = (296.0 + 0.25 * (np.arange(h) % 68))[:, None]
    dx[:, :4] = ramp
    dx[:, w - 4:] = ramp
    fx = _frame(dx, _random_sem(6, h, w, ncat, (1, 2, 5)))
    return [("limit_z", fz), ("limit_y", fy), ("limit_x", fx)]


# (name, start pose (x m, y m, heading deg), turn per frame in rad or None = the scene's own, frames)
POSE_STARTS = [
    ("wrap_pos", (12.0, 12.0, 179.0), math.radians(0.7), 3),          # crosses +180 -> -180 on the second frame
    ("wrap_neg", (12.0, 12.0, -179.5), -math.radians(0.7), 3),
    ("head_p180", (12.0, 12.0, 180.0), 0.0, 2),
    ("head_m180", (12.0, 12.0, -180.0), 0.0, 2),
    ("full_turn", (12.0, 12.0, 0.0), 2.0 * math.pi + 0.3, 2),
]
# (name, start pose, how much of the warped window lies inside the map: cut / full / none)
BORDER_STARTS = [
    ("sw_in", (0.4, 0.4, 0.0), "cut"), ("sw_out", (0.4, 0.4, 225.0 - 360.0), "none"),
    ("e_along", (23.9, 12.0, 90.0), "cut"), ("e_out", (23.9, 12.0, 0.0), "none"),     # along the edge: half the window is cut
    ("s_along", (12.0, 0.05, 0.0), "cut"), ("s_out", (12.0, 0.05, -90.0), "none"),
    ("ne_in", (23.9, 23.9, -135.0), "full"), ("ne_out", (23.9, 23.9, 45.0), "none"),    # from the corner inwards: all of it fits
    ("outside", (-3.0, 30.0, 0.0), "none"),
    ("far_outside", (1.0e10, -1.0e10, 30.0), "none"),          # sampling coordinates beyond the range of an int
]


def ordinary_frames(n: int = 3):
    """The ordinary scene every pose start drives (no stairs frame, no far band among its first three)."""
    return make_sequence(51, n)


def edge_scenes() -> List[Dict]:
    """Every edge scene: dict(name, frames, start = (x, y, heading), source = name of the scene whose depth / sem images
    it reuses or None).  Every scene starts from an empty map.  Depths are multiples of 1/4 cm except where a scene needs
    exact heights or weights (the stairs frames, limit_z, dense_order)."""
    S = []
    for p in stairs_pairs():
        for side in ("a", "b"):
            S.append(dict(name=f"stairs_{p['name']}_{side}", frames=[p[side]], start=CENTRE, source=None))
    S.append(dict(name="stairs_n0", frames=[stairs_empty_frame()], start=CENTRE, source=None))
    S.append(dict(name="dense_seq", frames=dense_sequence(), start=CENTRE, source=None))
    S.append(dict(name="dense_order", frames=[order_frame()], start=CENTRE, source=None))
    for name, fr in limit_frames():
        S.append(dict(name=name, frames=[fr], start=CENTRE, source=None))
    base = ordinary_frames()
    S.append(dict(name="ord", frames=[dict(f, pose=np.zeros(3, np.float32)) for f in base], start=CENTRE, source=None))
    for name, start, turn, n in POSE_STARTS:
        S.append(dict(name=f"pose_{name}", start=start, source="ord",
                      frames=[dict(f, pose=np.array([f["pose"][0], f["pose"][1], turn], np.float32)) for f in base[:n]]))
    for name, start, _ in BORDER_STARTS:
        S.append(dict(name=f"border_{name}", start=start, source="ord",
                      frames=[dict(f, pose=np.array([f["pose"][0], f["pose"][1], 0.0], np.float32)) for f in base[:2]]))
    return S
