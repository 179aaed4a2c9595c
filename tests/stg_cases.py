"""Cases of the short-term-goal tests (test infrastructure, importable without a GPU) and a NumPy restatement of the control flow of
the reference's ``Agent_Helper._get_stg`` (nav/agent/agent_helper.py:374-493).

tools/gen_golden_stg.py runs the reference's OWN code on these cases and writes tests/golden/stg_golden.npz; tests/test_stg_cpu.py
holds the restatement below to that file, tests/test_stg_gpu.py holds the device to it.

Three families:

* ``mask_cases()``   (a) every traversible map and goal mask ``_get_stg`` hands to its planner, with the planner's answers scripted so
  that the retry and 0 / 1 / 8 / 2 (toilet) magnify steps are all driven;
* ``window_cases()`` (b) float64 fields and states for ``FMMPlanner.get_short_term_goal``;
* ``scene_cases()``  (c) whole scenes: walls with doors, a goal behind a wall, an unreachable goal, a blocked start that needs the retry.
"""
import os

import numpy as np
from scipy import ndimage as ndi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stg_golden.npz")
STEP_SIZE = 5
MAGNIFY_WHEN_HARD = 100      # nav/arguments.py:96


def disk(r):
    """``skimage.morphology.disk``: x^2 + y^2 <= r^2."""
    r = int(r)
    L = np.arange(-r, r + 1)
    X, Y = np.meshgrid(L, L)
    return (X ** 2 + Y ** 2 <= r ** 2).astype(np.uint8)


def toilet_rule(goal_name):
    """(radius with found_goal, magnify steps): :425-430, :479."""
    return (6, 2) if goal_name == 'toilet' else (8, 8)


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def add_boundary(mat, value):
    h, w = mat.shape
    out = np.full((h + 2, w + 2), value, np.uint8)
    out[1:h + 1, 1:w + 1] = mat
    return out


def bordered_grid(obstacle, lmb, full_w, full_h):
    """rint(obstacle) != 0 with the four border rules (:382-390); ``grid[y1] = 1`` is a ROW, as the reference writes it."""
    gx1, gx2, gy1, gy2 = [int(v) for v in lmb]
    grid = np.rint(np.asarray(obstacle)) != 0
    if gx2 == full_w:
        grid[-1] = True
    if gy2 == full_h:
        grid[:, -1] = True
    if gx1 == 0:
        grid[0] = True
    if gy1 == 0:
        grid[0] = True
    return grid


def traversible(grid, lmb, col_rad, collision, visited, start, erode=False):
    """(:408-420) on the bordered grid, or (:448-461) on its erosion -> uint8 [(m + 2), (m + 2)]."""
    gx1, gx2, gy1, gy2 = [int(v) for v in lmb]
    if erode:
        grid = ndi.binary_erosion(grid, border_value=1)
    trav = ~ndi.binary_dilation(grid, structure=disk(col_rad))
    trav[collision[gx1:gx2, gy1:gy2] == 1] = False
    trav[visited[gx1:gx2, gy1:gy2] == 1] = True
    i, j = int(start[0]), int(start[1])
    trav[i - 1:i + 2, j - 1:j + 2] = True          # Python slices: [-1:2] selects nothing
    return add_boundary(trav.astype(np.uint8), 1)


def dilate_goal(padded, radius):
    return ndi.binary_dilation(padded != 0, structure=disk(radius)).astype(np.uint8)


def get_stg(case, plan):
    """``_get_stg``'s control flow.  ``plan(trav, goal, state) -> (stg_x, stg_y, distance, stop, replan)`` stands for
    ``FMMPlanner(trav)``, ``set_multi_goal(goal)``, ``get_short_term_goal(state)``.  Returns the result dict of
    ``peanut_amd.planner.ShortTermGoal`` plus every (trav, goal) pair handed to ``plan``."""
    m = case["m"]
    full = case["full"]
    found, (radius_found, max_magnify) = int(case["found_goal"]), toilet_rule(case["goal_name"])
    start = case["start_exact"]
    grid = bordered_grid(case["obstacle"], case["lmb"], full, full)
    trav = traversible(grid, case["lmb"], case["col_rad"], case["collision"], case["visited"], start)
    goal = dilate_goal(add_boundary(case["goal"], 0), radius_found if found == 1 else 2)
    state = [start[0] + 1, start[1] + 1]
    masks = [(trav, goal)]
    sx, sy, distance, stop, replan = plan(trav, goal, state)
    retried = 0
    if replan:
        retried = 1
        trav = traversible(grid, case["lmb"], case["col_rad"], case["collision"], case["visited"], start, erode=True)
        masks.append((trav, goal))
        sx, sy, distance, stop, replan = plan(trav, goal, state)
    n_magnify = 0
    if found == 1 and distance > case.get("magnify_when_hard", MAGNIFY_WHEN_HARD):
        step = 0
        while distance > 100:
            step += 1
            if step > max_magnify:
                break
            goal = dilate_goal(goal, 2)
            n_magnify += 1
            masks.append((trav, goal))
            sx, sy, distance, stop, replan = plan(trav, goal, state)
    return dict(stg=(float(sx) - 1, float(sy) - 1), distance=float(distance), stop=bool(stop), replan=bool(replan), retried=retried,
                n_magnify=n_magnify, n_solves=len(masks), masks=masks)


class Script:
    """A planner that answers ``get_short_term_goal`` from a list of (distance, replan); the last entry repeats."""

    def __init__(self, replies):
        self.replies, self.calls = list(replies), 0

    def __call__(self, trav, goal, state):
        d, rp = self.replies[min(self.calls, len(self.replies) - 1)]
        self.calls += 1
        return 10.0 + self.calls, 20.0 + self.calls, float(d), False, bool(rp)


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) mask cases
# ---------------------------------------------------------------------------------------------------------------------------------
OBST_VALUES = np.array([0.3, 0.5, 0.500001, 1.0, 1.5, 2.5], np.float32)      # rint: 0, 0 (half to even), 1, 1, 2, 2
SPECIAL = (0, 30, 31, 32, -1)

SCRIPTS = {
    "plain": ([(50, False)], 0, "chair", 0, 0),                       # replies, found_goal, goal_name, retried, n_magnify
    "retry": ([(50, True), (50, False)], 0, "chair", 1, 0),
    "found_near": ([(90, False)], 1, "chair", 0, 0),
    "mag1": ([(150, False), (90, False)], 1, "chair", 0, 1),
    "mag8": ([(150, False)], 1, "chair", 0, 8),
    "toilet": ([(150, False)], 1, "toilet", 0, 2),
    "retry_mag2": ([(150, True), (150, False), (150, False), (90, True)], 1, "bed", 1, 2),
    "unfound_far": ([(150, False)], 0, "toilet", 0, 0),
}


def window_bounds(pos, m, full):
    mid = (full - m) // 2
    gx1 = {"top": 0, "tl": 0, "bottom": full - m, "br": full - m}.get(pos, mid)
    gy1 = {"left": 0, "tl": 0, "right": full - m, "br": full - m}.get(pos, mid)
    return [gx1, gx1 + m, gy1, gy1 + m]


def mask_cases():
    cases = []
    positions = ["interior", "top", "bottom", "left", "right", "tl", "br"]
    starts = [(0, 0), (0, 1), (1, 0), (1, 1), (-1, -1), (-1, 7), (9, -1), (0, -1), (-1, 0), (20, 33)]
    names = list(SCRIPTS)
    for i in range(16):
        rng = np.random.RandomState(1000 + i)
        m = (61, 62, 45)[i % 3]
        full = 2 * m
        pos = positions[i % len(positions)]
        script = names[i % len(names)]
        replies, found, goal_name, _, _ = SCRIPTS[script]
        obstacle = np.where(rng.rand(m, m) < 0.012, rng.choice(OBST_VALUES, size=(m, m)), 0).astype(np.float32)
        goal = (rng.rand(m, m) < 0.002).astype(np.uint8)
        for k, a in enumerate(SPECIAL):        # obstacles and goal cells on the tile seams, the borders and in the corners
            for b in SPECIAL:
                if rng.rand() < 0.4:
                    obstacle[a, b] = OBST_VALUES[(i + k) % len(OBST_VALUES)]
                if rng.rand() < 0.3:
                    goal[a, b] = 1
        goal[(0, -1)[i % 2], (-1, 0)[(i // 2) % 2]] = 1
        lmb = window_bounds(pos, m, full)
        collision = (rng.rand(full, full) < 0.01).astype(np.uint8)
        visited = (rng.rand(full, full) < 0.01).astype(np.uint8)
        both = rng.rand(full, full) < 0.004        # the same cell in both: visited wins (the order of :412-414)
        collision[both] = 1
        visited[both] = 1
        collision[rng.rand(full, full) < 0.002] = 2      # only `== 1` counts
        s = starts[i % len(starts)]
        frac = [(0.0, 0.0), (0.5, 0.25), (0.999999, 0.125)][i % 3]
        start = [float(s[0] % m) + frac[0], float(s[1] % m) + frac[1]]
        cases.append(dict(name=f"a{i:02d}_{pos}_m{m}_r{(0, 1, 3, 4)[i % 4]}_{script}", m=m, full=full, lmb=lmb, col_rad=(0, 1, 3, 4)[i % 4],
                          obstacle=obstacle, goal=goal, collision=collision, visited=visited, start_exact=start, found_goal=found,
                          goal_name=goal_name, script=script))
    return cases


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) window cases: (name, field key, state)
# ---------------------------------------------------------------------------------------------------------------------------------
def window_fields():
    n = 63
    r, c = np.mgrid[0:n, 0:n].astype(np.float64)
    f = {}
    f["euclid"] = np.sqrt((r - 50.3) ** 2 + (c - 11.7) ** 2) * 1.0371
    f["manhattan"] = np.abs(r - 40) + np.abs(c - 40)                  # exact ties in every window
    pl = f["euclid"].copy()                                           # plateaus of max + 1, as ma.filled leaves them
    top = pl.max() + 1
    pl[20:30, 15:40] = top
    pl[0:4, :] = top
    pl[:, 59:] = top
    f["plateau"] = pl
    flat = np.full((n, n), 7.25)                                      # nothing lower than the centre anywhere
    f["flat"] = flat
    near5 = f["manhattan"].copy() * 0.5 + 30
    near5[30, 30] = np.nextafter(5.0, 0.0)                            # a centre at 4.999... (stop) ...
    near5[30, 40] = 5.0                                               # ... and at 5.0 exactly (no stop)
    f["near5"] = near5
    thr = np.full((n, n), 3.0)                                        # centres at 0: the window's minimum is the field's own value
    thr[:, 0:21] = -0.0001
    thr[:, 21:42] = np.nextafter(-0.0001, 0.0)
    thr[:, 42:] = np.nextafter(-0.0001, -1.0)
    thr[10::10, 5::21] = 0.0
    f["threshold"] = thr
    thr8 = np.full((n, n), 9.0)                                       # the same around a centre at 8: (8 - 0.0001) - 8 and neighbours
    v = 8.0 - 0.0001
    thr8[:, 0:21], thr8[:, 21:42], thr8[:, 42:] = v, np.nextafter(v, 9.0), np.nextafter(v, 0.0)
    thr8[10::10, 5::21] = 8.0
    f["threshold8"] = thr8
    nan = f["euclid"].copy()
    nan[33, 28] = nan[31, 33] = np.nan                                # two NaNs on the ring of the window at (30, 30): the first wins
    nan[45, 45] = np.nan                                              # a NaN centre
    f["nan"] = nan
    small = (np.abs(np.mgrid[0:7, 0:7][0] - 1.0) * 1.5 + np.abs(np.mgrid[0:7, 0:7][1] - 5.0)).astype(np.float64)
    f["small"] = small                                                # n = 7: the pad value enters on every side
    return f


def window_cases():
    cases = []
    fr = [0.0, 0.5, 0.999999, 0.25]
    for k, (a, b) in enumerate([(30, 30), (0, 0), (0, 62), (62, 0), (62, 62), (3, 31), (31, 4), (58, 31), (31, 59), (5, 5), (57, 57),
                                (22, 18), (25, 41), (17, 30), (45, 45), (1, 61)]):
        for name in ("euclid", "manhattan", "plateau", "nan"):
            cases.append((f"{name}_{a}_{b}", name, (a + fr[k % 4], b + fr[(k + 1) % 4])))
    for b in (30, 40):
        for k in range(4):
            cases.append((f"near5_{b}_{k}", "near5", (30 + fr[k], b + fr[(k + 2) % 4])))
    for name in ("threshold", "threshold8"):
        for a in (10, 20, 30):
            for b in (5, 26, 47):
                cases.append((f"{name}_{a}_{b}", name, (a + 0.5, b + 0.5)))
                cases.append((f"{name}_{a}_{b}_int", name, (float(a), float(b))))
    for a, b in [(31, 31), (0, 5), (62, 62)]:
        cases.append((f"flat_{a}_{b}", "flat", (a + 0.5, b + 0.125)))
    for a in range(0, 7, 2):
        for b in range(0, 7, 3):
            cases.append((f"small_{a}_{b}", "small", (a + 0.75, b + 0.5)))
    return cases


def mask_sweep():
    """Fractional parts for get_mask / get_dist, including the values at which a cell's d2 sits on a circle."""
    v = [0.0, 0.5, 0.25, 0.75, 0.1, 0.3, 0.7, 0.9, 0.999999, 1e-9, 1.0 - 2.0 ** -53, 1.0 / 3.0, 0.6180339887498949]
    return [(a, b) for a in v for b in v]


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) scenes
# ---------------------------------------------------------------------------------------------------------------------------------
# The device field may sit up to 0.5 cell from the oracle's (tests/test_goal_gpu.py), so every decision of a scene needs a margin of
# a whole cell (tools/gen_golden_stg.py: check_margins).  On open floor neighbouring cells of the window's ring differ by less than
# that; the scenes therefore walk corridors ONE cell wide, where the ring meets the free space in two cells five steps apart.
def _carve(free, pts):
    """Axis-aligned polyline of free cells through ``pts``."""
    for (r0, c0), (r1, c1) in zip(pts[:-1], pts[1:]):
        assert r0 == r1 or c0 == c1
        free[min(r0, r1):max(r0, r1) + 1, min(c0, c1):max(c0, c1) + 1] = True


def _scene(name, m, pos, col_rad, start, found, goal_name, goal_cell, retry, magnify):
    full = 2 * m
    c = dict(name=name, m=m, full=full, lmb=window_bounds(pos, m, full), col_rad=col_rad, obstacle=np.zeros((m, m), np.float32),
             goal=np.zeros((m, m), np.uint8), collision=np.zeros((full, full), np.uint8), visited=np.zeros((full, full), np.uint8),
             start_exact=[float(start[0]), float(start[1])], found_goal=found, goal_name=goal_name, expect_retry=retry,
             expect_magnify=magnify)
    c["goal"][goal_cell] = 1
    return c


def _local(c, key):
    gx1, gx2, gy1, gy2 = c["lmb"]
    return c[key][gx1:gx2, gy1:gy2]


def scene_cases():
    out = []
    # walls with two doors: everything but the walk is obstacle; the long-term goal cell (nothing found) three rooms away
    c = _scene("doors", 61, "interior", 0, (14.5, 8.5), 0, "chair", (50, 52), 0, 0)
    free = np.zeros((61, 61), bool)
    _carve(free, [(4, 8), (50, 8), (50, 30), (10, 30), (10, 52), (50, 52)])
    c["obstacle"][~free] = 1.5
    out.append(c)
    # a found chair behind a wall: obstacles dilated by the collision disk, the door through the thickened wall kept open by the
    # visited trail; the window touches the top and left borders of the full map (rows 0..3 blocked by the border rule)
    c = _scene("behind_wall", 62, "tl", 3, (20.5, 10.25), 1, "chair", (30, 52), 0, 0)
    free = np.zeros((62, 62), bool)
    _carve(free, [(8, 10), (50, 10), (50, 40), (30, 40), (30, 52)])
    c["obstacle"][~ndi.binary_dilation(free, structure=disk(3))] = 1
    c["obstacle"][45:56, 25] = 1                                     # a wall across the walk ...
    _local(c, "visited")[50, 18:33] = 1                              # ... and the trail through it
    out.append(c)
    # a found toilet in a closed room: never reached, neither before nor after the erosion (the rock between is eleven cells thick)
    c = _scene("unreachable", 45, "br", 1, (8.5, 12.5), 1, "toilet", (32, 30), 1, 0)
    free = np.zeros((45, 45), bool)
    _carve(free, [(8, 6), (8, 38)])
    _carve(free, [(24, 22), (40, 22), (40, 38), (24, 38), (24, 22)])
    c["obstacle"][~ndi.binary_dilation(free, structure=disk(1))] = 1
    out.append(c)
    # the walls are the collision map (the erosion does not touch them); one obstacle cell plugs the walk and the erosion removes it
    c = _scene("blocked_start", 61, "right", 1, (30.5, 12.5), 0, "bed", (12, 50), 1, 0)
    free = np.zeros((61, 61), bool)
    _carve(free, [(30, 4), (30, 33), (12, 33), (12, 50)])
    _local(c, "collision")[~free] = 1
    c["obstacle"][30, 25] = 0.500001
    out.append(c)
    # a found toilet at the end of a serpentine, farther than 100 cells: two magnify steps (the toilet's limit) leave it there
    free = np.zeros((62, 62), bool)
    _carve(free, [(4, 4), (56, 4), (56, 20), (6, 20), (6, 36), (56, 36), (56, 52), (20, 52)])
    c = _scene("serpentine_toilet", 62, "bottom", 0, (10.5, 4.5), 1, "toilet", (20, 52), 0, 2)
    c["obstacle"][~free] = 1
    out.append(c)
    # the same walk for a chair: eight steps, the limit
    c = _scene("serpentine_chair", 62, "bottom", 0, (10.5, 4.5), 1, "chair", (20, 52), 0, 8)
    c["obstacle"][~free] = 1
    out.append(c)
    # ... and a goal whose disk, grown twice, reaches the lane next to it: the distance falls from far above 100 to far below
    c = _scene("serpentine_shortcut", 62, "bottom", 0, (30.5, 4.5), 1, "chair", (30, 32), 0, None)
    c["obstacle"][~free] = 1
    out.append(c)
    return out


