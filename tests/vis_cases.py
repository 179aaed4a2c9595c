"""Cases of the visualisation tests (test infrastructure, importable without a GPU): deterministic inputs for the reference's
``Agent_Helper._visualize`` (nav/agent/agent_helper.py:496-621) and a NumPy restatement of it.

tools/gen_golden_vis.py runs the reference's OWN ``_visualize`` / ``init_vis_image`` / ``get_contour_points`` on ``golden_cases()``
and writes tests/golden/vis_golden.npz (expected index maps, frames WITHOUT the arrow, the arrow's vertices and colour, the file
name); it also holds ``restate`` below to the reference on every one of them.  tests/test_vis_cpu.py checks what each case claims
to contain on those arrays; tests/test_vis_gpu.py holds the device renderer to them bit for bit.

UNPINNED (cv2 is absent where the fixture is made) and therefore tested against the restatement only: the arrow's fill
(``fill_polygon``) and the nearest resize at ratios that are not exact (``nearest_index`` at m = 100).

Inputs are patterns, not random numbers, so that the stored frames compress."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vis_golden.npz")
H, W = 600, 1415
RES = 5
# values around the rint thresholds of `np.rint(x) == 1` (half to even: 0.5 -> 0, 1.5 -> 2)
RINT_TABLE = np.array([0.0, 0.4, 0.5, 0.6, 1.0, 1.5, 2.5, 1.4999], np.float32)


def disk(radius):
    L = np.arange(-radius, radius + 1)
    X, Y = np.meshgrid(L, L)
    return (X ** 2 + Y ** 2) <= radius ** 2


def legend():
    """A patterned BGR legend [40, 300, 3]."""
    i, j = np.mgrid[0:40, 0:300]
    return np.stack([(i * 6) % 256, (j // 10 * 8) % 256, ((i // 8 + j // 25) * 40) % 256], axis=2).astype(np.uint8)


def rgb_frame(k=0):
    """A patterned RGB observation [480, 640, 3] (blocks and ramps; the three channels differ so that a missed flip shows)."""
    i, j = np.mgrid[0:480, 0:640]
    return np.stack([(j // 16 * 6 + k) % 256, (i // 16 * 8) % 256, ((i // 32 + j // 32) * 23 + 5 * k) % 256], axis=2).astype(np.uint8)


def _fields(m, kind, bits):
    """target_pred (float32, or float64 holding float32 values), value, dd_wt (float64) [m, m]."""
    i, j = np.mgrid[0:m, 0:m].astype(np.float64)
    # k / 96 for k = 0..96: normed = x exactly; x * 256 is an integer for every k divisible by 3; the extremes are 0 and 1
    tp = (((i * 5 + j * 7) % 97) / 96.0).astype(np.float32)
    if kind == "f32edge":
        # min 0.3f, max 0.67f: the span is no power of two, so the float division rounds; `edge_values` go onto white cells later
        tp = (np.float32(0.3) + np.float32(0.37) * (((i * 5 + j * 7) % 97) / 96.0).astype(np.float32)).astype(np.float32)
    dd = np.exp(-np.hypot(i - m / 3.0, j - m / 4.0) / (m / 2.0 + 1.0))
    value = tp.astype(np.float64) * dd
    if kind == "const":
        dd = np.full((m, m), 0.25)                      # max == min: 0 / 0, the "bad" colour everywhere
    if kind == "nan":
        value = value.copy()
        value[m // 2, m // 3] = np.nan                  # one NaN: np.min is NaN, the whole panel is "bad"
    if kind == "inf":
        dd = dd.copy()
        dd[0, 0] = np.inf                               # max = inf: finite cells -> 0, the cell itself inf / inf -> "bad"
    return (tp.astype(np.float64) if bits == 64 else tp), value, dd


def edge_values(lo, hi, count=48):
    """float32 values x in (lo, hi) whose colour index differs between the two arithmetics: ``(x - lo) / (hi - lo) * 256`` truncates
    to k - 1 in double and to k in float (the float quotient rounds up onto k / 256) or the other way round.  Found by search among
    the float32 neighbours of lo + (hi - lo) * k / 256; the order is that of k."""
    lo, hi = np.float32(lo), np.float32(hi)
    found = []
    for k in range(1, 256):
        x = np.float32(np.float64(lo) + (np.float64(hi) - np.float64(lo)) * k / 256.0)
        for _ in range(3):
            x = np.nextafter(x, np.float32(-np.inf))
        for _ in range(7):
            f = int((x - lo) / (hi - lo) * np.float32(256))
            d = int((np.float64(x) - np.float64(lo)) / (np.float64(hi) - np.float64(lo)) * 256.0)
            if f != d and lo < x < hi:
                found.append(x)
                break
            x = np.nextafter(x, np.float32(np.inf))
        if len(found) == count:
            break
    return np.array(found, np.float32)


def make_case(name, m, ncat, full, origin, stg, pose, fields="plain", bits=32, rgb=0, claims=()):
    """One case: the maps of an episode whose m x m local window starts at ``origin`` of a ``full`` x ``full`` map."""
    gx1, gy1 = origin
    C = 4 + ncat
    I, J = np.mgrid[0:full, 0:full]
    full_map = np.zeros((C, full, full), np.float32)
    full_map[0] = RINT_TABLE[(I * 3 + J) % 8]
    full_map[1] = RINT_TABLE[(I + 2 * J) % 8]
    full_map[2] = ((I + J) % 5) / 4.0
    full_map[3] = ((I * J) % 3) / 2.0
    for c in range(ncat - 1):
        full_map[4 + c] = ((I * 7 + J * 13 + c * 5) % 11) / 10.0
    full_map[4 + ncat - 1] = 7.0                        # the last plane is REPLACED by 1e-5 before the arg-max: never wins by this
    i, j = I - gx1, J - gy1                             # window coordinates
    for c in range(ncat - 1):                           # every category wins somewhere (with ncat = 22: indices beyond the palette)
        full_map[4 + c][((i % 6) >= 3) & ((j // 4) % ncat == c)] = 5.0
    # a band where every category plane is 0 (arg-max = the last plane: no category)
    band = ((i % 6) < 3) if m >= 6 else ((i + j) % 2 == 0)
    full_map[4:4 + ncat - 1, band] = 0.0
    collision = np.zeros((full, full), np.uint8)
    visited = np.zeros((full, full), np.uint8)
    collision[(I % 9 == 4) & (J % 7 == 3)] = 1          # falls into the band and outside it
    collision[(I * 5 + J) % 61 == 0] = 1
    visited[(I == J + (gx1 - gy1) + 2) & (I % 4 != 0)] = 1      # a dashed diagonal through the window
    goal = np.zeros((m, m), np.uint8)
    if m >= 16:
        for r, c in ((0, 0), (0, m // 2), (m - 1, m // 3), (m // 2, 0), (m // 2 + 3, m - 1), (m - 2, m - 2), (m // 2, m // 2), (m // 2, m // 2 + 1)):
            goal[r, c] = 1
        visited[gx1 + m // 2 + 2, gy1 + m // 2 + 2] = 1          # a visited cell inside the goal's dilation: the goal wins (:543)
        visited[gx1 + m // 2 + 9, gy1 + m // 2] = 1              # and one outside it
    else:
        goal[0, 0] = 1                                  # the map is smaller than the disk(4) footprint
    # two cells that nothing later overrides: in the band, plane 2 equal to 1e-5f exactly (a tie with the replaced last plane: the
    # FIRST maximum, plane 2, wins); outside it, planes 1 and 3 tied at the top (plane 1 wins)
    tie_cell = tie13_cell = None
    if m >= 16:
        from scipy import ndimage as ndi
        win = (slice(gx1, gx1 + m), slice(gy1, gy1 + m))
        free = ~((collision[win] == 1) | (visited[win] == 1) | ndi.binary_dilation(goal != 0, structure=disk(4)))
        if stg is not None and -m <= int(stg[0]) < m and -m <= int(stg[1]) < m:
            free[int(stg[0]), int(stg[1])] = False
        free[:6] = False
        tie_cell = tuple(int(v) for v in np.argwhere(free & band[win])[0])
        tie13_cell = tuple(int(v) for v in np.argwhere(free & ~band[win])[0])
        full_map[4 + 2, gx1 + tie_cell[0], gy1 + tie_cell[1]] = np.float32(1e-5)
        full_map[4 + 1, gx1 + tie13_cell[0], gy1 + tie13_cell[1]] = full_map[4 + 3, gx1 + tie13_cell[0], gy1 + tie13_cell[1]] = 9.0
    tp, value, dd = (None, None, None) if fields is None else _fields(m, fields, bits)
    if fields == "f32edge":
        # the overlay shows only where the map's colour is pure white (index 0): the edge values go onto such cells, so that the
        # arithmetic's width decides pixels of the frame
        assert bits == 32 and tp.dtype == np.float32
        probe = dict(m=m, ncat=ncat, lmb=[gx1, gx1 + m, gy1, gy1 + m], full_map=full_map, collision=collision, visited=visited, goal=goal, stg=stg)
        white = np.argwhere(index_map(probe) == 0)
        lo, hi = tp.min(), tp.max()
        edges = edge_values(lo, hi)
        assert len(edges) >= 8 and len(white) >= 4 * len(edges), (len(edges), len(white))
        for k, x in enumerate(edges):
            r, q = white[3 * k + 5]
            tp[r, q] = x
        assert tp.min() == lo and tp.max() == hi
        value = tp.astype(np.float64) * dd
    return dict(name=name, m=m, ncat=ncat, full=full, lmb=[gx1, gx1 + m, gy1, gy1 + m], full_map=full_map, collision=collision,
                visited=visited, goal=goal, stg=stg, pose=tuple(float(v) for v in pose), target_pred=tp, value=value, dd_wt=dd,
                bits=bits, rgb=None if rgb is None else rgb_frame(rgb), goal_name="chair" if ncat == 10 else "tv_monitor",
                rank=ncat % 3, episode_no=2 + m % 5, timestep=m % 97 + 1, tie_cell=tie_cell, tie13_cell=tie13_cell,
                claims=tuple(claims))


def pose_at(m, origin, frac_r, frac_c, o):
    """A pose whose window cell is (frac_r * m, frac_c * m): x runs along columns, y along rows (agent_helper.py:264-268)."""
    return ((origin[1] + frac_c * m) * RES / 100.0, (origin[0] + frac_r * m) * RES / 100.0, o)


def golden_cases():
    """The cases tests/golden/vis_golden.npz holds (sizes as the issue's table; every setting at a small size)."""
    out = [
        make_case("m480_view", 480, 10, 960, (240, 200), (-1, 2), pose_at(480, (240, 200), 0.5, 0.5, 30.0), bits=64,
                  claims=("collapse14", "stg_wraps", "goal_borders", "all_zero", "tie_1e5", "visited_over_goal", "normed_0_1", "integer_scaled")),
        make_case("m240_x2", 240, 16, 240, (0, 0), (240, 3), pose_at(240, (0, 0), 0.25, 0.7, -100.0), bits=32,
                  claims=("no_collapse14", "stg_skipped", "goal_borders", "all_zero", "tie_1e5", "visited_over_goal", "normed_0_1", "integer_scaled")),
        make_case("m96_x5", 96, 22, 192, (96, 0), (40.9, 41.2), pose_at(96, (96, 0), 0.8, 0.1, 170.0), bits=64, rgb=3,
                  claims=("no_collapse14", "beyond_palette", "goal_borders", "all_zero", "tie_1e5", "visited_over_goal")),
        make_case("m96_nopred", 96, 10, 96, (0, 0), (5, 96), pose_at(96, (0, 0), 0.5, 0.5, 0.0), fields=None, rgb=None,
                  claims=("collapse14", "stg_skipped", "no_pred", "rgb_none")),
        make_case("m96_const", 96, 10, 96, (0, 0), (7, 9), pose_at(96, (0, 0), 0.3, 0.6, 45.0), fields="const", bits=32,
                  claims=("collapse14", "black_dd_wt")),
        make_case("m96_nan", 96, 16, 96, (0, 0), (-96, -1), pose_at(96, (0, 0), 0.6, 0.3, 200.0), fields="nan", bits=32, rgb=None,
                  claims=("stg_wraps", "black_value", "rgb_none")),
        make_case("m96_inf", 96, 10, 96, (0, 0), (95, 95), pose_at(96, (0, 0), 0.5, 0.2, 90.0), fields="inf", bits=64,
                  claims=("collapse14",)),
        make_case("m96_f32", 96, 10, 128, (16, 24), (30, 31), pose_at(96, (16, 24), 0.7, 0.7, -20.0), fields="f32edge", bits=32,
                  claims=("collapse14", "float_differs")),
        make_case("m8", 8, 10, 16, (8, 4), (-1, -8), pose_at(8, (8, 4), 0.5, 0.5, 10.0), bits=64, claims=("stg_wraps", "small")),
        make_case("m8_c16", 8, 16, 8, (0, 0), (8, 0), pose_at(8, (0, 0), 0.2, 0.9, -45.0), bits=32, claims=("stg_skipped", "small")),
        make_case("m1", 1, 10, 2, (1, 1), (0, 0), pose_at(1, (1, 1), 0.5, 0.5, 0.0), bits=64, claims=("small", "black_dd_wt", "black_value")),
        make_case("m1_nopred", 1, 16, 1, (0, 0), (1, 1), pose_at(1, (0, 0), 0.5, 0.5, 0.0), fields=None, claims=("small", "no_pred", "stg_skipped")),
    ]
    return out


REQUIRED_CLAIMS = ("collapse14", "no_collapse14", "stg_skipped", "stg_wraps", "goal_borders", "all_zero", "tie_1e5", "visited_over_goal",
                   "normed_0_1", "integer_scaled", "beyond_palette", "no_pred", "rgb_none", "black_dd_wt", "black_value", "small", "float_differs")


def resize_case():
    """m = 100: 4.8 and 2.4 are not exact ratios; against the restatement only."""
    return make_case("m100", 100, 10, 200, (37, 61), (50, 50), pose_at(100, (37, 61), 0.4, 0.4, 60.0), bits=64)


def arrow_cases():
    """(name, arrow [4, 2]) for the arrow tests, as (x, y) frame pixels: at the map panel's corners, partly outside the frame,
    with two coinciding vertices, degenerate."""
    def dart(x, y):
        return [[x, y], [x - 4, y - 7], [x + 12, y], [x - 4, y + 7]]
    return [("panel_top_left", dart(670, 50)), ("panel_bottom_right", dart(1149, 529)), ("leaves_left_top", dart(-3, 2)),
            ("leaves_right_bottom", dart(1410, 597)), ("outside", dart(-40, -40)),
            ("coinciding", [[700, 100], [700, 100], [712, 100], [696, 107]]), ("all_one_point", [[800, 300]] * 4),
            ("flat", [[900, 200], [905, 200], [912, 200], [903, 200]]), ("bow_tie", [[1000, 400], [1020, 420], [1020, 400], [1000, 420]])]


# ---- the restatement ----
def sem_argmax(local_map):
    """``vlm = clone(local_map[4:]); vlm[-1] = 1e-5; vlm.argmax(0)`` (agent_state.py:259-262); np.argmax: the first maximum."""
    vlm = np.array(local_map[4:], np.float32)
    vlm[-1] = np.float32(1e-5)
    return np.argmax(vlm, axis=0).astype(np.int64)


def index_map(case):
    """:512-543 -> int64 [m, m]."""
    from scipy import ndimage as ndi
    m, ncat = case["m"], case["ncat"]
    gx1, gx2, gy1, gy2 = case["lmb"]
    lm = case["full_map"][:, gx1:gx2, gy1:gy2]
    sem = sem_argmax(lm) + 5
    sem[case["collision"][gx1:gx2, gy1:gy2] == 1] = 14
    if case["stg"] is not None and int(case["stg"][0]) < m and int(case["stg"][1]) < m:
        sem[int(case["stg"][0]), int(case["stg"][1])] = 15
    no_cat = sem == ncat + 4
    sem[no_cat] = 0
    sem[no_cat & (np.rint(lm[1]) == 1)] = 2
    sem[no_cat & (np.rint(lm[0]) == 1)] = 1
    sem[case["visited"][gx1:gx2, gy1:gy2] == 1] = 3
    sem[ndi.binary_dilation(case["goal"] != 0, structure=disk(4))] = 4
    return sem


def nearest_index(dst_n, src_n):
    """cv2's legacy INTER_NEAREST along one axis: ``min(int(floor(dst * ifx)), n - 1)``, ``ifx = 1.0 / (dst_n / src_n)`` in double."""
    ifx = 1.0 / (float(dst_n) / float(src_n))
    return np.minimum(np.floor(np.arange(dst_n, dtype=np.float64) * ifx).astype(np.int64), src_n - 1)


def colour_index(x):
    """Entry of the 257-entry table for every cell of a field, in the field's own dtype (:565-567 and matplotlib's Colormap.__call__)."""
    with np.errstate(all="ignore"):
        normed = (x - np.min(x)) / (np.max(x) - np.min(x))
        xa = normed * normed.dtype.type(256)
        idx = np.where(np.isnan(xa), 256, np.where(xa == 256, 255, np.nan_to_num(xa).astype(np.int64)))
    return idx


def fill_polygon(pts, shape=(H, W)):
    """The pixels whose integer centre lies in the closed polygon ``pts`` [(x, y)]: on an edge, or inside by crossing number
    (even-odd), in exact integer arithmetic -> bool [H, W]."""
    pts = [(int(x), int(y)) for x, y in pts]
    mask = np.zeros(shape, bool)
    x0, x1 = max(min(p[0] for p in pts), 0), min(max(p[0] for p in pts), shape[1] - 1)
    y0, y1 = max(min(p[1] for p in pts), 0), min(max(p[1] for p in pts), shape[0] - 1)
    for y in range(y0, y1 + 1):
        for x in range(x0, x1 + 1):
            crossings, on_edge = 0, False
            for k in range(len(pts)):
                (ax, ay), (bx, by) = pts[k], pts[(k + 1) % len(pts)]
                cross = (bx - ax) * (y - ay) - (x - ax) * (by - ay)
                if cross == 0 and min(ax, bx) <= x <= max(ax, bx) and min(ay, by) <= y <= max(ay, by):
                    on_edge = True
                elif (ay > y) != (by > y):
                    # the edge meets the row of y at ax + (y - ay) * (bx - ax) / (by - ay); strictly right of x?
                    num, den = (y - ay) * (bx - ax) - (x - ax) * (by - ay), by - ay
                    crossings += (num > 0) == (den > 0)
            mask[y, x] = on_edge or crossings % 2 == 1
    return mask


def restate(case, background, palette, cmap, arrow=None, arrow_bgr=None):
    """The whole frame (:545-608) from ``index_map(case)`` -> uint8 [600, 1415, 3]; ``palette`` uint8 [256, 3] RGB, ``cmap`` uint8
    [257, 3] BGR.  ``arrow``: vertices to fill with ``arrow_bgr``, or None."""
    m = case["m"]
    img = background.copy()
    sem = index_map(case)
    vis = palette[sem.astype(np.uint8)][::-1][:, :, ::-1]                 # palette, flipud, BGR
    big = nearest_index(480, m)
    vis = vis[big][:, big]
    if case["rgb"] is not None:
        img[50:530, 15:655] = case["rgb"][:, :, ::-1]
    img[50:530, 670:1150] = vis
    if case["target_pred"] is not None:
        overlay = cmap[colour_index(case["target_pred"])][::-1][big][:, big]
        white = vis.astype(np.int64).sum(axis=2) == 765
        img[50:530, 670:1150][white] = overlay[white]
        small = nearest_index(240, m)
        img[290:530, 1165:1405] = cmap[colour_index(case["value"])][::-1][small][:, small]
        img[50:290, 1165:1405] = cmap[colour_index(case["dd_wt"])][::-1][small][:, small]
        img[49, 1165:1405] = 100
        img[530, 1165:1405] = 100
        img[49:531, 1405] = 100
    if arrow is not None:
        img[fill_polygon(arrow)] = arrow_bgr
    return img
