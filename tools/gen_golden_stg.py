"""Writes tests/golden/stg_golden.npz: what the reference's OWN ``Agent_Helper._get_stg`` (nav/agent/agent_helper.py:374-493) and
``FMMPlanner.get_short_term_goal`` / ``get_mask`` / ``get_dist`` (nav/agent/utils/fmm_planner.py:8-36, 77-116) give on the cases of
tests/stg_cases.py.

The reference's agent/agent_helper.py and agent/utils/fmm_planner.py are imported at run time, unmodified, under empty stand-in
modules for what is absent (cv2, skfmm, skimage, torchvision, agent.utils.segmentation); ``skimage.morphology`` is bound to the scipy
calls scikit-image itself makes: ``binary_dilation(image, footprint)`` -> ``ndi.binary_dilation(image, structure=footprint)``,
``binary_erosion(image)`` -> ``ndi.binary_erosion(image, border_value=1)``, ``disk(r)`` = x^2 + y^2 <= r^2.  ``_get_stg`` is called
unbound on a stand-in object with the fields it reads.

(a) masks: ``agent_helper.FMMPlanner`` is a recording subclass that stores every traversible map and goal mask it is handed and
    answers ``get_short_term_goal`` from the case's script.
(b) windows: the reference's ``get_short_term_goal`` on stored fields and states, and ``get_mask`` / ``get_dist`` over a sweep.
(c) scenes: the whole ``_get_stg`` with ``skfmm.distance`` bound to oracle/fmm_ref.distance (PARITY UNPINNED, as that file says).
    The device field may differ from that oracle by up to the 0.5-cell gate of tests/test_goal_gpu.py, so a scene is admitted only
    if every decision ``_get_stg`` takes on it has a margin of more than 1.0 cell (``check_margins``).  Exempt are the comparisons
    that involve no solver arithmetic: two window cells that both lie on the field's fill plateau (``ma.filled(dd, max + 1)`` writes
    ONE value into every masked or unreached cell, in any solver, and which cells those are is topology) are equal on both sides,
    and plateau minus plateau is exactly 0 on both sides.

Needs the reference checkout (it does not travel with the tests; the .npz does).

    python -m tools.gen_golden_stg
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
from scipy import ndimage as ndi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import stg_cases as sc                              # noqa: E402
from oracle import fmm_ref, ref_import              # noqa: E402


def load_reference():
    nav = os.path.join(ref_import.REF, "nav")
    if nav not in sys.path:
        sys.path.insert(0, nav)
    for name in ("cv2", "skfmm", "skimage", "torchvision", "agent.utils.segmentation"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torchvision"].transforms = types.ModuleType("torchvision.transforms")
    sys.modules["agent.utils.segmentation"].SemanticPredMaskRCNN = object
    morph = types.ModuleType("skimage.morphology")
    morph.binary_dilation = lambda image, footprint=None: ndi.binary_dilation(image, structure=footprint)
    morph.binary_erosion = lambda image: ndi.binary_erosion(image, border_value=1)
    morph.disk = lambda r: sc.disk(r)
    sys.modules["skimage.morphology"] = morph
    sys.modules["skimage"].morphology = morph
    sys.modules["skfmm"].distance = fmm_ref.distance
    import matplotlib
    matplotlib.use("Agg")
    import agent.agent_helper as ah                 # type: ignore
    import agent.utils.fmm_planner as fp            # type: ignore
    return ah, fp


def call_get_stg(ah, case, planner_cls):
    """The reference's ``_get_stg`` on a case -> ((stg_x, stg_y), stop), the planners it made, next_preset_goal calls."""
    made, preset = [], []

    class Planner(planner_cls):
        def __init__(self, traversible, *a, **k):
            super().__init__(traversible, *a, **k)
            made.append(self)

    ah.FMMPlanner = Planner
    gx1, gx2, gy1, gy2 = case["lmb"]
    me = types.SimpleNamespace(full_w=case["full"], full_h=case["full"], selem=sc.disk(case["col_rad"]), collision_map=case["collision"].copy(),
                               visited_vis=case["visited"].copy(), found_goal=case["found_goal"], info={"goal_name": case["goal_name"]},
                               args=types.SimpleNamespace(only_explore=1, magnify_goal_when_hard=case.get("magnify_when_hard", sc.MAGNIFY_WHEN_HARD)),
                               agent_states=types.SimpleNamespace(next_preset_goal=lambda: preset.append(1)))
    grid = np.rint(case["obstacle"])                # _plan :251
    start = [np.float64(case["start_exact"][0]), np.float64(case["start_exact"][1])]      # pose_pred is an ndarray: numpy scalars (:257-266)
    stg, stop = ah.Agent_Helper._get_stg(me, grid, start, np.copy(case["goal"]).astype(np.float64), [gx1, gx2, gy1, gy2])
    return stg, stop, made, len(preset)


def recording_planner(fp, replies):
    script = sc.Script(replies)

    class Recording(fp.FMMPlanner):
        def __init__(self, traversible, *a, **k):
            super().__init__(traversible, *a, **k)
            self.goals = []

        def set_multi_goal(self, goal_map):
            self.goals.append(np.array(goal_map))

        def get_short_term_goal(self, state):
            return script(self.traversible, self.goals[-1], state)

    return Recording, script


def solving_planner(fp):
    class Solving(fp.FMMPlanner):
        def __init__(self, traversible, *a, **k):
            super().__init__(traversible, *a, **k)
            self.goals, self.fields, self.answers = [], [], []

        def set_multi_goal(self, goal_map):
            self.goals.append(np.array(goal_map))
            super().set_multi_goal(goal_map)
            self.fields.append((np.array(self.fmm_dist), np.array(np.ma.getmaskarray(np.ma.masked_values(self.traversible * 1, 0)))))

        def get_short_term_goal(self, state):
            out = super().get_short_term_goal(state)
            self.answers.append((out, [float(s) for s in state]))
            return out

    return Solving


def u8(mask):
    a = np.asarray(mask)
    assert np.isin(a, (0, 1)).all()
    return a.astype(np.uint8)


def check_margins(fp, name, field, state, magnify_when_hard, found):
    """Every decision taken on this solve keeps more than 1.0 cell (0.2 for the ratio) from its threshold; see the module docstring
    for the two exemptions."""
    n, du = field.shape[0], sc.STEP_SIZE
    ir, ic = int(state[0]), int(state[1])
    mask = fp.get_mask(state[0] - ir, state[1] - ic, 1.0, sc.STEP_SIZE)
    dist_mask = fp.get_dist(state[0] - ir, state[1] - ic, 1.0, sc.STEP_SIZE)
    pad = np.pad(field, du, 'constant', constant_values=n ** 2)
    raw = pad[ir:ir + 2 * du + 1, ic:ic + 2 * du + 1].copy()
    top = field.max()
    unreached = (np.pad(field, du, 'constant', constant_values=-1)[ir:ir + 2 * du + 1, ic:ic + 2 * du + 1] == top) & (np.sum(field == top) > 1)
    centre = raw[du, du]
    sub = raw * mask + (1 - mask) * n ** 2 - centre
    ratio = sub / dist_mask
    ring = mask == 1
    assert np.all(np.abs(ratio[ring] + 1.5) > 0.2), f"{name}: a ratio within 0.2 of -1.5"
    sub[ratio < -1.5] = 1
    order = np.argsort(sub, axis=None, kind="stable")
    best, second = np.unravel_index(order[0], sub.shape), np.unravel_index(order[1], sub.shape)
    plateau_tie = unreached[best] and unreached[second] and unreached[du, du]
    assert plateau_tie or sub[second] - sub[best] > 1.0, f"{name}: the best cell leads by {sub[second] - sub[best]}"
    assert (unreached[best] and unreached[du, du] and sub[best] == 0) or abs(sub[best] + 0.0001) > 1.0, f"{name}: minimum {sub[best]}"
    assert abs(centre - 5.0) > 1.0, f"{name}: centre {centre}"
    assert abs(centre - 100) > 1.0 and abs(centre - magnify_when_hard) > 1.0, f"{name}: distance {centre}"
    return dict(lead=float(sub[second] - sub[best]), minimum=float(sub[best]), centre=float(centre), plateau=bool(plateau_tie))


def generate():
    ah, fp = load_reference()
    out = {}
    # ---- (a) ----
    for c in sc.mask_cases():
        replies, _, _, want_retry, want_magnify = sc.SCRIPTS[c["script"]]
        cls, script = recording_planner(fp, replies)
        stg, stop, made, preset = call_get_stg(ah, c, cls)
        pairs = [(u8(p.traversible), u8(g)) for p in made for g in p.goals]
        mine = sc.get_stg(c, sc.Script(replies))
        assert len(pairs) == mine["n_solves"] == script.calls and mine["retried"] == want_retry == preset and mine["n_magnify"] == want_magnify, c["name"]
        for k, ((t, g), (mt, mg)) in enumerate(zip(pairs, mine["masks"])):
            assert np.array_equal(t, mt) and np.array_equal(g, mg), f"{c['name']}: the restatement's masks of solve {k} differ"
            out[f"a/{c['name']}/trav{k}"], out[f"a/{c['name']}/goal{k}"] = t, g
        assert tuple(float(v) for v in stg) == mine["stg"]
        out[f"a/{c['name']}/n"] = np.array([len(pairs), want_retry, want_magnify], np.int64)
        for key in ("obstacle", "goal", "collision", "visited"):
            out[f"a/{c['name']}/{key}"] = c[key]
        out[f"a/{c['name']}/params"] = np.array([c["m"], c["full"], *c["lmb"], c["col_rad"], c["found_goal"]], np.int64)
        out[f"a/{c['name']}/start"] = np.array(c["start_exact"], np.float64)
        print(f"[stg a] {c['name']:44s} solves {len(pairs)} retry {want_retry} magnify {want_magnify}")
    # ---- (b) ----
    fields = sc.window_fields()
    for k, f in fields.items():
        out[f"b/field/{k}"] = f
    rows = []
    for name, key, state in sc.window_cases():
        p = fp.FMMPlanner(np.ones_like(fields[key]), step_size=sc.STEP_SIZE)
        p.fmm_dist = fields[key].copy()
        sx, sy, distance, stop, replan = p.get_short_term_goal([np.float64(state[0]), np.float64(state[1])])
        rows.append([state[0], state[1], float(sx), float(sy), float(distance), float(bool(stop)), float(bool(replan))])
    out["b/results"] = np.array(rows, np.float64)
    r = out["b/results"]
    print(f"[stg b] {len(rows)} windows: stop {int(r[:, 5].sum())}, replan {int(r[:, 6].sum())}, NaN distance {int(np.isnan(r[:, 4]).sum())}")
    sweep = sc.mask_sweep()
    out["b/sweep"] = np.array(sweep, np.float64)
    out["b/get_mask"] = np.array([fp.get_mask(np.float64(a), np.float64(b), 1.0, sc.STEP_SIZE) for a, b in sweep])
    out["b/get_dist"] = np.array([fp.get_dist(np.float64(a), np.float64(b), 1.0, sc.STEP_SIZE) for a, b in sweep])
    assert all(np.array_equal(fp.get_mask(a, b, 1.0, 5), fp.get_mask(np.float64(a), np.float64(b), 1.0, 5)) and
               np.array_equal(fp.get_dist(a, b, 1.0, 5), fp.get_dist(np.float64(a), np.float64(b), 1.0, 5)) for a, b in sweep)
    # ---- (c) ----
    for c in sc.scene_cases():
        stg, stop, made, preset = call_get_stg(ah, c, solving_planner(fp))
        solves = [(p, k) for p in made for k in range(len(p.goals))]
        mag = c.get("magnify_when_hard", sc.MAGNIFY_WHEN_HARD)
        notes = [check_margins(fp, c["name"], p.fields[k][0], p.answers[k][1], mag, c["found_goal"]) for p, k in solves]
        retried, n_magnify = int(len(made) == 2), len(solves) - len(made)
        last = made[-1].answers[-1][0]

        def plan(trav, goal, state, fp=fp):
            q = fp.FMMPlanner(trav.astype(np.float64), step_size=sc.STEP_SIZE)
            q.set_multi_goal(goal.astype(np.float64))
            return q.get_short_term_goal([np.float64(state[0]), np.float64(state[1])])
        mine = sc.get_stg(c, plan)
        assert mine["stg"] == tuple(float(v) for v in stg) and mine["stop"] == bool(stop) and mine["retried"] == retried == preset and \
            mine["n_magnify"] == n_magnify, c["name"]
        assert retried == c["expect_retry"] and (c["expect_magnify"] is None or n_magnify == c["expect_magnify"]), (c["name"], retried, n_magnify)
        out[f"c/{c['name']}/result"] = np.array([stg[0], stg[1], float(bool(stop)), retried, n_magnify, len(solves), float(last[2]), float(bool(last[4]))], np.float64)
        print(f"[stg c] {c['name']:20s} stg {tuple(float(v) for v in stg)} stop {bool(stop)} retry {retried} magnify {n_magnify} "
              f"distances {[round(n['centre'], 2) for n in notes]} leads {[round(n['lead'], 2) for n in notes]}")
    np.savez_compressed(sc.GOLDEN, **out)
    print(f"[stg] -> {sc.GOLDEN} ({os.path.getsize(sc.GOLDEN)} bytes)")


if __name__ == "__main__":
    generate()
