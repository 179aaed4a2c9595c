"""Cases of the motion-planner tests (test infrastructure, importable without a GPU): chains of steps for the reference's
``Agent_Helper.plan_act`` / ``_plan`` (nav/agent/agent_helper.py:130-159, :228-371) with the short-term goal scripted, so that no
solver arithmetic enters and every comparison is exact.

tools/gen_golden_plan.py runs the reference's OWN code on these chains and writes tests/golden/plan_golden.npz;
tests/test_plan_cpu.py checks what every chain claims to exercise against that file (``CLAIMS``), tests/test_plan_gpu.py holds
``peanut_amd.agent_helper.Agent_Helper`` to it.

A chain: ``cfg`` (``num_sem_categories``, ``move_forward_after_stop``, ``global_downscaling``, ``seed`` of the global NumPy RNG;
the full map is 96 x 96 cells of 5 cm) and ``steps``: per step the pose ``(x, y, o)`` in metres / degrees, the window ``lmb``, the
scripted ``(stg, stop)`` and ``found_goal``.  The poses are scripted too: they are the world's answer to the previous action, and a
chain may answer a forward action with no motion (a bump)."""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_golden.npz")
FULL = 96                       # cells; map_size_cm = 480, map_resolution = 5
RES = 5
TURN_ANGLE = 30
COLLISION_THRESHOLD = 0.20
# the columns of a golden "state" row
STATE = ("action", "col_width", "prev_blocked", "forward_after_stop", "previous_action", "last_action", "total_id", "epi_id", "timestep",
         "last_start_r", "last_start_c", "n_collision", "n_visited")
W_LOW, W_MID, W_HIGH = [0, 48, 0, 48], [24, 72, 24, 72], [48, 96, 48, 96]
W_ALL = [0, 96, 0, 96]


def cfg_args(cfg):
    """The arguments a chain runs under, as a dict (the reference's names)."""
    return dict(map_size_cm=FULL * RES, map_resolution=RES, global_downscaling=cfg["global_downscaling"],
                num_sem_categories=cfg["num_sem_categories"], move_forward_after_stop=cfg["move_forward_after_stop"],
                turn_angle=TURN_ANGLE, collision_threshold=COLLISION_THRESHOLD, col_rad=4, only_explore=1, visualize=0,
                magnify_goal_when_hard=100)


def local_size(cfg):
    return int(FULL / cfg["global_downscaling"])


def cell(pose, lmb):
    """The unthresholded window cell of a pose (agent_helper.py:267-268)."""
    x, y = np.float64(pose[0]), np.float64(pose[1])
    return [int(y * 100.0 / RES - lmb[0]), int(x * 100.0 / RES - lmb[2])]


def ahead(pose, lmb, m, d=8):
    """A short-term goal ``d`` cells straight ahead of the pose's heading: the planner answers "forward"."""
    r, c = cell(pose, lmb)
    r, c = min(max(r, 0), m - 1), min(max(c, 0), m - 1)
    o = math.radians(pose[2])
    return (float(r + round(d * math.sin(o))), float(c + round(d * math.cos(o))))


def step(pose, lmb, stg, stop=0, found=0):
    return dict(pose=tuple(float(v) for v in pose), lmb=list(lmb), stg=(float(stg[0]), float(stg[1])), stop=int(stop), found=int(found))


def _walk_edges():
    """The visited line with a point on row 0, on column 0, at m - 1, and last_start == start."""
    cfg = dict(num_sem_categories=10, move_forward_after_stop=1, global_downscaling=2, seed=1)
    poses = [(0.02, 1.0, 0.0), (1.0, 0.01, 90.0), (1.0, 0.01, 90.0), (2.39, 2.39, 0.0), (1.2, 1.2, 200.0), (0.02, 0.02, 10.0)]
    return cfg, [step(p, W_LOW, (24.0, 30.0)) for p in poses]


def _window_moves():
    """The window moves between steps: last_start is formed in the NEW window and clamped there."""
    cfg = dict(num_sem_categories=10, move_forward_after_stop=1, global_downscaling=2, seed=1)
    seq = [((2.4, 2.4, 0.0), W_MID), ((3.0, 3.0, 0.0), W_LOW), ((3.0, 3.0, 0.0), W_HIGH), ((1.0, 1.0, 0.0), W_HIGH),
           ((1.3, 1.1, 45.0), W_LOW), ((3.5, 3.6, 45.0), W_MID)]
    return cfg, [step(p, w, (20.0, 30.0)) for p, w in seq]


def _blocked():
    """Forward actions without motion: ``buf`` 4 -> 2 past ``block_threshold``, the untrap sequence past 30 tries (the global RNG),
    an unblock, and a second block with the sides swapped.  The agent turns in place through the headings 0, 30, 45, 90, 180, 270,
    -30 and 400 degrees while it is stuck."""
    cfg = dict(num_sem_categories=10, move_forward_after_stop=1, global_downscaling=2, seed=1234)
    headings = [0.0, 30.0, 45.0, 90.0, 180.0, 270.0, -30.0, 400.0]
    steps = []
    for k in range(76):                                     # stuck at (1.2, 1.2): 4 bumps, then an untrap try every second step
        p = (1.2, 1.2, headings[(k // 2) % len(headings)])
        steps.append(step(p, W_LOW, ahead(p, W_LOW, 48)))
    for x in (1.45, 1.2, 1.45, 1.2):                        # free again: 0.25 m per step, to and fro (the edge buffer keeps every
        p = (x, 1.2, 0.0)                                   # "ahead" goal honest only near the middle of the window)
        steps.append(step(p, W_LOW, ahead(p, W_LOW, 48)))
    for k in range(18):                                     # the second block
        p = (1.2, 1.2, headings[(k // 2) % len(headings)])
        steps.append(step(p, W_LOW, ahead(p, W_LOW, 48)))
    return cfg, steps


def _border():
    """17 categories (edge_buffer 40), one window over the whole map: bumps beside the map border, where the collision cells are
    clamped, and short-term goals outside the edge-buffer band on each side.  So close to the border the edge buffer steers every
    short-term goal inwards; the forward actions that bump come from the stop countdown (stop and found_goal on every step:
    forward, stop, forward, ...)."""
    cfg = dict(num_sem_categories=17, move_forward_after_stop=1, global_downscaling=1, seed=1)
    steps = []
    for p in [(4.75, 0.02, 0.0), (4.75, 0.02, 0.0), (4.75, 0.02, 0.0),            # heading +x at the far column: c clamps to 95
              (0.1, 4.71, 180.0), (0.1, 4.71, 180.0), (0.1, 4.71, 180.0),           # heading -x at column 2: c clamps to 0
              (2.01, 0.1, 270.0), (2.01, 0.1, 270.0), (2.01, 0.1, 270.0),           # heading -y at row 2: r clamps to 0
              (2.01, 4.75, 90.0), (2.01, 4.75, 90.0), (2.01, 4.75, 90.0)]:          # heading +y at the far row: r clamps to 95
        steps.append(step(p, W_ALL, ahead(p, W_ALL, 96), stop=1, found=1))
    for stg in [(5.0, 90.0), (90.0, 5.0), (39.0, 56.0), (40.0, 55.0), (48.0, 48.0)]:
        steps.append(step((2.4, 2.4, 0.0), W_ALL, stg))
    return cfg, steps


def _thresholds():
    """A forward action followed by |dx| (|dy|) on each side of 0.05 and by a distance on each side of collision_threshold."""
    cfg = dict(num_sem_categories=10, move_forward_after_stop=1, global_downscaling=2, seed=1)
    x, y = 1.2, 1.2
    # (never four bumps in a row: the untrap override would take the forward actions away)
    # (and to and fro, so that the agent stays where the edge buffer leaves the goal ahead of it alone)
    moves = [(0.0, 0.0), (0.049, 0.0), (-0.25, 0.0), (0.051, 0.0), (0.21, 0.0), (0.0, 0.049), (-0.19, 0.0), (0.0, -0.051), (0.25, 0.0),
             (-0.14, -0.14), (0.15, 0.15), (-0.049, -0.049), (0.0, -0.21), (0.0, 0.0), (-0.2, 0.0), (0.0, 0.25)]
    steps = []
    for dx, dy in moves:
        x, y = x + dx, y + dy
        p = (x, y, 0.0)
        steps.append(step(p, W_LOW, ahead(p, W_LOW, 48)))
    return cfg, steps


def _stop(k):
    """``stop`` with found_goal 0 / 1 under move_forward_after_stop = k, through the countdown and its negative reset, twice."""
    cfg = dict(num_sem_categories=10, move_forward_after_stop=k, global_downscaling=2, seed=1)
    script = [(0, 0), (1, 0), (0, 1), (1, 1), (1, 1), (1, 1), (1, 1), (0, 0), (1, 1), (0, 1), (0, 0), (1, 0), (1, 1), (1, 1), (1, 1), (0, 0)]
    steps = []
    for k, (stop, found) in enumerate(script):
        p = ((1.2, 1.45)[k % 2], 1.2, 0.0)                   # the world moves the agent whatever it did: no bump in this chain
        steps.append(step(p, W_LOW, ahead(p, W_LOW, 48), stop, found))
    return cfg, steps


def _angles():
    """Relative angles equal to +turn_angle / 2 and -turn_angle / 2 (forward), just beyond each, across +-180, and headings above
    360 and below 0.  The agent stands on cell (24, 24) of its window; a goal at (24, 24 + d) lies at exactly 0 degrees."""
    cfg = dict(num_sem_categories=10, move_forward_after_stop=1, global_downscaling=2, seed=1)
    east, west_up, west_down, north = (24.0, 34.0), (25.0, 11.0), (23.0, 11.0), (34.0, 24.0)
    seq = [(15.0, east), (-15.0, east), (15.000001, east), (-15.000001, east), (375.0, east), (375.000001, east), (345.0, east), (-375.0, east),
           (90.0, east), (270.0, east), (180.0, east), (-180.0, east), (176.0, west_down), (-176.0, west_up), (181.0, west_up),
           (179.5, west_down), (105.0, north), (75.0, north), (105.000001, north), (74.999999, north), (400.0, east), (-30.0, east)]
    # two places 1.7 m apart that are both cell (24, 24) of their window, in turn: no step is a bump
    places = [((1.225, 1.225), W_LOW), ((2.425, 2.425), W_MID)]
    return cfg, [step(places[k % 2][0] + (o,), places[k % 2][1], stg) for k, (o, stg) in enumerate(seq)]


def chains():
    out = {"walk_edges": _walk_edges(), "window_moves": _window_moves(), "blocked": _blocked(), "border": _border(),
           "thresholds": _thresholds(), "angles": _angles()}
    for k in (0, 1, 2):
        out[f"stop{k}"] = _stop(k)
    return {name: dict(name=name, cfg=cfg, steps=steps) for name, (cfg, steps) in out.items()}


# ---------------------------------------------------------------------------------------------------------------------------------
# what the chains claim, checked on the fixture (tests/test_plan_cpu.py)
# ---------------------------------------------------------------------------------------------------------------------------------
def line(last_start, start):
    """``vu.draw_line``'s points (utils/visualization.py:19-24), the NumPy expression."""
    return [(int(np.rint(last_start[0] + (start[0] - last_start[0]) * i / 25)), int(np.rint(last_start[1] + (start[1] - last_start[1]) * i / 25)))
            for i in range(26)]


def starts(chain):
    """Per step (last_start, start) as ``_plan`` forms them (:267-277): thresholded cells of the current window."""
    m = local_size(chain["cfg"])
    out, last = [], (FULL * RES / 100.0 / 2.0, FULL * RES / 100.0 / 2.0, 0.0)
    for s in chain["steps"]:
        clamp = lambda rc: [min(max(0, rc[0]), m - 1), min(max(0, rc[1]), m - 1)]
        out.append((clamp(cell(last, s["lmb"])), clamp(cell(s["pose"], s["lmb"]))))
        last = s["pose"]
    return out


def relative_angle(chain, k):
    s = chain["steps"][k]
    _, start = starts(chain)[k]
    goal = math.degrees(math.atan2(s["stg"][0] - start[0], s["stg"][1] - start[1]))
    agent = s["pose"][2] % 360.0
    if agent > 180:
        agent -= 360
    rel = (agent - goal) % 360.0
    return rel - 360 if rel > 180 else rel


def col(state, name):
    return state[:, STATE.index(name)]


def claim_walk_edges(chain, g):
    m = local_size(chain["cfg"])
    pts = [p for ls, st in starts(chain) for p in line(ls, st)]
    assert any(x == 0 for x, _ in pts) and any(y == 0 for _, y in pts) and any(x == m - 1 and y == m - 1 for x, y in pts)
    assert any(ls == st for ls, st in starts(chain))
    assert [list(r) for r in g["state"][:, 9:11]] == [ls for ls, _ in starts(chain)]


def claim_window_moves(chain, g):
    m = local_size(chain["cfg"])
    steps = chain["steps"]
    moved = [k for k in range(1, len(steps)) if steps[k]["lmb"] != steps[k - 1]["lmb"]]
    assert len(moved) >= 3
    clamped = [k for k in moved if not all(0 <= v < m for v in cell(steps[k - 1]["pose"], steps[k]["lmb"]))]
    assert clamped, "no step whose last position leaves the new window"
    assert [list(r) for r in g["state"][:, 9:11]] == [ls for ls, _ in starts(chain)]


def claim_blocked(chain, g):
    st = g["state"]
    assert col(st, "prev_blocked").max() >= 30 and col(st, "epi_id").max() > 30
    assert set(col(st, "total_id")) == {0, 1}
    second = st[col(st, "total_id") == 1]
    assert col(second, "epi_id").max() >= 3 and col(second, "prev_blocked").max() >= 5
    first = st[(col(st, "total_id") == 0) & (col(st, "epi_id") > 0)]
    # the sides: tries 1-2 and 19-30 one way, 3-18 the other, swapped in the second block; past 30 both turns occur
    by_try = lambda rows, lo, hi: {int(a) for a, e, p in zip(col(rows, "action"), col(rows, "epi_id"), col(rows, "previous_action")) if lo <= e <= hi and a != 1}
    assert by_try(first, 1, 2) == {2} and by_try(first, 3, 18) == {3} and by_try(first, 19, 30) == {2} and by_try(first, 31, 99) == {2, 3}
    assert by_try(second, 1, 2) == {3} and by_try(second, 3, 18) == {2}
    # buf 4 before the threshold, 2 after it: heading 0 at x = 1.2 m marks columns 28, 29 and later 26, 27
    cm = g["collision"]
    assert cm[1][24, 28] == 1 and cm[1][24, 29] == 1 and cm[1][24, 26] == 0
    headings = {s["pose"][2] for s in chain["steps"]}
    assert {0.0, 30.0, 45.0, 90.0, 180.0, 270.0, -30.0, 400.0} <= headings


def claim_border(chain, g):
    cm = g["collision"][-1]
    assert cm[0, 95] == 1 and cm[94, 0] == 1 and cm[0, 40] == 1 and cm[95, 40] == 1
    assert chain["cfg"]["num_sem_categories"] == 17
    band = (40, 96 - 40 - 1)
    stgs = [s["stg"] for s in chain["steps"][-5:]]
    assert any(s[0] < band[0] for s in stgs) and any(s[0] > band[1] for s in stgs) and any(s[1] < band[0] for s in stgs) and any(s[1] > band[1] for s in stgs)


def claim_thresholds(chain, g):
    steps, st = chain["steps"], g["state"]
    dxs = [(abs(np.float64(a["pose"][0]) - np.float64(b["pose"][0])), abs(np.float64(a["pose"][1]) - np.float64(b["pose"][1])))
           for a, b in zip(steps[:-1], steps[1:])]
    assert any(0 < dx < 0.05 for dx, _ in dxs) and any(0.05 <= dx < 0.06 for dx, _ in dxs)
    assert any(0 < dy < 0.05 for _, dy in dxs) and any(0.05 <= dy < 0.06 for _, dy in dxs)
    dist = [float((dx ** 2 + dy ** 2) ** 0.5) for dx, dy in dxs]
    assert any(0.18 < d < COLLISION_THRESHOLD for d in dist) and any(COLLISION_THRESHOLD <= d < 0.22 for d in dist)
    # a bump raises prev_blocked, a free move clears it: both happen after forward actions
    pb = col(st, "prev_blocked")
    assert pb.max() >= 2 and (np.diff(pb) < 0).any()


def claim_stop(chain, g):
    k = chain["cfg"]["move_forward_after_stop"]
    st = g["state"]
    fas, act = col(st, "forward_after_stop"), col(st, "action")
    assert fas.max() == k and (0 in act)
    if k > 0:
        low = np.where(fas[:-1] == -1)[0]
        assert len(low) >= 2 and (fas[low + 1] >= k - 1).all()                        # the negative reset on the next step
    stops = [(s["stop"], s["found"]) for s in chain["steps"]]
    assert {(0, 0), (1, 0), (0, 1), (1, 1)} <= set(stops)


def claim_angles(chain, g):
    rel = [relative_angle(chain, k) for k in range(len(chain["steps"]))]
    act = [int(a) for a in col(g["state"], "action")]
    half = TURN_ANGLE / 2.
    assert rel[0] == half and rel[1] == -half and act[0] == act[1] == 1
    assert 0 < rel[2] - half < 1e-5 and act[2] == 3 and 0 < -half - rel[3] < 1e-5 and act[3] == 2
    assert any(abs(r) < half and abs(s["pose"][2]) > 170 for r, s in zip(rel, chain["steps"]))      # across +-180: still forward
    for r, a in zip(rel, act):
        assert a == (3 if r > half else 2 if r < -half else 1)
    assert {2, 3, 1} == set(act)


CLAIMS = {"walk_edges": claim_walk_edges, "window_moves": claim_window_moves, "blocked": claim_blocked, "border": claim_border,
          "thresholds": claim_thresholds, "stop0": claim_stop, "stop1": claim_stop, "stop2": claim_stop, "angles": claim_angles}


def load_golden():
    z = np.load(GOLDEN)
    return {name: {k: z[f"{name}/{k}"] for k in ("state", "visited", "collision")} for name in chains()}
