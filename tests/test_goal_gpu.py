"""Long-term goal selection on the device (csrc/goal.hip, peanut_amd/goal.py) against
oracle/fmm_ref.c (restated scikit-fmm, PARITY UNPINNED), oracle/goal_ref.py and the golden episode produced by the
reference's own Agent_State.update_global_goal (tests/golden/goal_golden.npz).

Gates: distance field <= 0.5 cell max-abs vs the heap-ordered oracle (measured: ~1e-12 on these maps), identical
masked / unreachable pattern, chosen goal cell identical; the field is the fixed point of its own scheme to 1.5e-6 cell
(oracle/goal_ref.fmm_fixed_point_residual) and the selection equals oracle/goal_ref.select_from_field on the device's field
(value map within 2 ulp, weight sum within 1e-12 relative, same keep-last decision and goal)."""
import os

import numpy as np
import pytest
import torch
from numpy import ma

pytestmark = pytest.mark.gpu

FIELD_TOL = 0.5      # cells (the gate); printed maxima show how far below it the solver sits


class FakePredictionGPU:
    """Device twin of oracle.agent_ref.FakePrediction (same formula on HIP tensors)."""

    def __init__(self, pattern):
        self.pattern = torch.from_numpy(pattern).cuda()

    def get_prediction_batch(self, maps, apply_sigmoid=True, out=None):
        sel = maps[:, [0, 1, 4, 5, 6, 7]]
        return torch.tanh(sel + self.pattern[None]) * 0.5 + 0.5


def _maze(h, w, seed, density=0.012, wall_len=(10, 60)):
    rng = np.random.RandomState(seed)
    trav = np.ones((h, w), np.uint8)
    for _ in range(int(density * h * w / 20)):
        r, c = rng.randint(0, h), rng.randint(0, w)
        n = rng.randint(*wall_len)
        if rng.rand() < 0.5:
            trav[r:r + 2, c:c + n] = 0
        else:
            trav[r:r + n, c:c + 2] = 0
    trav[rng.randint(0, h, 40), rng.randint(0, w, 40)] = 0
    if h >= 40 and w >= 40:
        # a closed box: its inside is unreachable
        trav[h // 4:h // 4 + 30, w // 4] = 0
        trav[h // 4:h // 4 + 30, w // 4 + 29] = 0
        trav[h // 4, w // 4:w // 4 + 30] = 0
        trav[h // 4 + 29, w // 4:w // 4 + 30] = 0
    return trav


def _ulp_gap(a, b):
    """Largest distance between a and b in units of the last place (of the larger magnitude); equal NaN / inf positions count 0."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b)), "NaN pattern"
    ok = ~np.isnan(a)
    a, b = a[ok], b[ok]
    same = a == b
    if same.all():
        return 0.0
    a, b = a[~same], b[~same]
    assert np.isfinite(a).all() and np.isfinite(b).all(), "infinite on one side only"
    return float((np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))).max())


def _select_and_check(sol, last, obst, col, vis, lmb, loc, tp, temperature, map_resolution=5):
    """One ``select`` held to oracle/goal_ref.select_from_field applied to the device's own field: value map within 2 ulp, sum of
    the weights within 1e-12 relative, the keep-last decision equal, the goal cell equal (unless the two best reference values are
    within 1e-15 relative: then one of them).  ``last`` = the weights the restatement carries from the previous call (``dd_wt``);
    returns (device result, the weights carried to the next call).  The device forgets the last weights when the window changes
    size (the reference would fail to broadcast them), and at temperature 0 -- where the reference's weights exp(-dd / 0) are
    never used -- it reports the sum of the frontier values and leaves the last weights alone."""
    from oracle import goal_ref
    lw, lh = lmb[1] - lmb[0], lmb[3] - lmb[2]
    if last is not None and last.shape != (lw, lh):
        last = None
    got = sol.select(obst, col, vis, lmb, loc, tp, temperature, map_resolution, want_dist=True, want_value=True)
    dd = got["dist"].cpu().numpy()
    tpn = None if tp is None else tp.detach().cpu().numpy().astype(np.float32)
    goal, value, wt_sum, kept, new_last = goal_ref.select_from_field(dd, lmb, tpn, temperature, map_resolution, last)
    v = got["value"].cpu().numpy()
    assert _ulp_gap(v, value) <= 2, f"value map: {_ulp_gap(v, value)} ulp"
    if temperature == 0:
        assert not got["kept_last"]
        wt_sum, new_last = float(np.sum(value)), last
    else:
        assert got["kept_last"] == kept, (got["kept_last"], kept, wt_sum)
    if np.isfinite(wt_sum) and wt_sum != 0.0:
        assert abs(got["wt_sum"] - wt_sum) <= 1e-12 * abs(wt_sum), (got["wt_sum"], wt_sum)
    else:
        assert got["wt_sum"] == wt_sum or (np.isnan(got["wt_sum"]) and np.isnan(wt_sum)), (got["wt_sum"], wt_sum)
    flat = value.ravel()
    top = flat[np.argmax(flat)]
    if got["goal"] != goal:
        assert np.isfinite(top) and top != 0.0
        near = np.flatnonzero(np.abs(flat - top) <= 1e-15 * abs(top))
        assert near.size >= 2 and np.ravel_multi_index(got["goal"], value.shape) in near, (got["goal"], goal)
    r, c = got["goal"]
    assert 0 <= r < lw and 0 <= c < lh
    assert np.array_equal(np.float64(got["value_max"]), v[r, c], equal_nan=True)
    return got, new_last


def _oracle_field(trav, seeds):
    from oracle import fmm_ref
    t = ma.masked_values(trav.astype(np.float64), 0)
    for r, c in seeds:
        t[r, c] = 0
    d = fmm_ref.distance(t, dx=1)
    return np.where(ma.getmaskarray(d), np.inf, ma.getdata(d))


@pytest.mark.parametrize("shape,seed", [((960, 960), 1), ((480, 480), 2), ((250, 333), 3), ((64, 40), 4)],
                         ids=lambda v: str(v))
def test_fmm_field_matches_oracle(shape, seed):
    from peanut_amd.goal import GeodesicSolver
    h, w = shape
    trav = _maze(h, w, seed)
    src = (h // 2 + 3, w // 2 - 5)
    trav[src[0] - 2:src[0] + 3, src[1] - 2:src[1] + 3] = 1
    ref = _oracle_field(trav, [src])
    sol = GeodesicSolver(h, w, 0)
    got = sol.distance(torch.from_numpy(trav), goal=src).cpu().numpy()
    assert np.array_equal(np.isinf(got), np.isinf(ref)), "masked / unreachable pattern"
    fin = np.isfinite(ref)
    assert fin.sum() > (0.5 if h > 100 else 0.2) * h * w
    if h > 100:
        assert np.isinf(ref[h // 4 + 10, w // 4 + 10]), "the closed box must stay unreached"
    err = np.abs(got[fin] - ref[fin]).max()
    print(f"{h}x{w}: max |GPU - oracle| = {err:.3e} cells over {fin.sum()} reached cells, max distance {ref[fin].max():.1f}, "
          f"{sol.rounds} relaxation rounds in {sol.passes} ordering passes, converged={sol.converged}")
    assert err <= FIELD_TOL
    assert sol.converged, "the ordering passes run to their fixed point under the default ceiling (24)"
    assert sol.passes < 24
    # fill_max_plus_one = ma.filled(dd, np.max(dd) + 1) (fmm_planner.py:66)
    filled = sol.distance(torch.from_numpy(trav), goal=src, fill_max_plus_one=True).cpu().numpy()
    assert np.isfinite(filled).all() and abs(filled[~fin].min() - (ref[fin].max() + 1)) <= FIELD_TOL
    assert np.unique(filled[~fin]).size == 1


def test_fmm_multi_goal_and_seed_inside_obstacle():
    from oracle import goal_ref
    from peanut_amd.goal import FMMPlanner, GeodesicSolver
    trav = _maze(300, 300, 9)
    gm = np.zeros((300, 300), np.uint8)
    gm[40:43, 200:203] = 1
    gm[250, 30] = 1
    gm[80, 80] = 1
    trav[80, 80] = 0                                    # a goal on a masked cell gets unmasked (traversible_ma[goal] = 0)
    ref = goal_ref.fmm_set_multi_goal(trav.astype(np.float64), gm)
    pl = FMMPlanner(trav.astype(np.float64))
    pl.set_multi_goal(gm)
    assert np.abs(pl.fmm_dist - ref).max() <= FIELD_TOL
    pl.set_goal((150.7, 149.2))
    ref1 = goal_ref.fmm_set_goal(trav.astype(np.float64), (150, 149))
    assert np.abs(pl.fmm_dist - ref1).max() <= FIELD_TOL
    # short-term goal: one step of descent on the field from a cell 30 cells away
    start = [150.4, 119.6]
    if trav[150, 119]:
        sx, sy, dist, stop, replan = pl.get_short_term_goal(start)
        assert not stop and pl.fmm_dist[int(sx), int(sy)] <= pl.fmm_dist[150, 119]
    # agent walled in: only the seed is reached
    box = np.zeros((64, 64), np.uint8)
    sol = GeodesicSolver(64, 64, 0)
    got = sol.distance(torch.from_numpy(box), goal=(10, 12)).cpu().numpy()
    assert got[10, 12] == 0 and np.isinf(got).sum() == 64 * 64 - 1


def test_fmm_adjacent_seeds_match_the_oracle():
    """Goal blobs (set_multi_goal): next to adjacent equal seeds the second-order term takes the second seed (`<=` in
    updatePointOrderTwo), e.g. 2/3 instead of 1 in line with a pair.  GPU field vs the restatement on open ground and in
    a maze, seeds as a 1x2 pair, a 3x3 block and an L."""
    from oracle import goal_ref
    from peanut_amd.goal import FMMPlanner
    for trav in (np.ones((96, 128), np.uint8), _maze(200, 200, 5)):
        gm = np.zeros(trav.shape, np.uint8)
        gm[40, 60:62] = 1
        gm[70:73, 20:23] = 1
        gm[20:23, 100] = 1
        gm[22, 100:103] = 1
        trav = trav.copy()
        trav[gm == 1] = 1
        ref = goal_ref.fmm_set_multi_goal(trav.astype(np.float64), gm)
        pl = FMMPlanner(trav.astype(np.float64))
        pl.set_multi_goal(gm)
        got = pl.fmm_dist
        if trav[40, 62] and trav[40, 59]:
            assert abs(ref[40, 62] - 2.0 / 3.0) < 1e-9 and abs(got[40, 62] - 2.0 / 3.0) < 1e-6
        near = np.zeros(trav.shape, bool)                 # cells within 3 steps of a seed: held tighter than the field
        ys, xs = np.nonzero(gm)
        for y, x in zip(ys, xs):
            near[max(0, y - 3):y + 4, max(0, x - 3):x + 4] = True
        assert np.abs(got - ref)[near].max() <= 0.05, np.abs(got - ref)[near].max()
        assert np.abs(got - ref).max() <= FIELD_TOL


def test_traversible_map_is_bit_exact():
    from oracle import goal_ref
    from oracle.agent_ref import disk
    from peanut_amd.goal import GeodesicSolver
    rng = np.random.RandomState(0)
    obst = (rng.rand(200, 260) > 0.97).astype(np.float32) * rng.choice([0.3, 0.5, 0.51, 1.0, 1.5], size=(200, 260)).astype(np.float32)
    obst[0, 0] = obst[199, 259] = 1.0                    # borders: the footprint is cut off, zero outside
    col = (rng.rand(200, 260) > 0.995).astype(np.float64)
    vis = (rng.rand(200, 260) > 0.99).astype(np.float64)
    for rad in (4, 1, 0, 7, 16, 17):          # (<= 16: row bit masks; beyond: the cell-by-cell footprint test)
        sol = GeodesicSolver(200, 260, rad)
        got = sol.traversible(torch.from_numpy(obst), col, vis).cpu().numpy()
        ref = goal_ref.traversible_map(obst, disk(rad), col, vis)
        assert np.array_equal(got.astype(bool), ref), rad


def test_goal_selection_episode_matches_reference(golden_dir):
    """The golden episode (reference Agent_State.update_global_goal under the restated skfmm): identical goal cell
    at every prediction step, incl. the 'avoid repeating the last goal' bookkeeping; distance probes and the
    last field within the gate."""
    from oracle import goal_ref, mapping_scenes
    from oracle.agent_ref import agent_args, fake_pattern
    from oracle.gen_golden_goal import helper_maps
    from peanut_amd.agent_state import Agent_State
    z = np.load(os.path.join(golden_dir, "goal_golden.npz"))
    args = agent_args(dist_weight_temperature=500, select_goal=False)
    st = Agent_State(args, prediction_model=FakePredictionGPU(fake_pattern(size=args.prediction_window)))
    frames = mapping_scenes.make_sequence(seed=int(z["seed"]), n_frames=int(z["n_frames"]))
    for f in frames:
        f["pose"][0] = np.float32(f["pose"][0] * 3.0)
    st.reset()
    col, vis = helper_maps((st.full_w, st.full_h), seed=int(z["helper_seed"]))
    st.collision_map.copy_(torch.from_numpy(col.astype(np.uint8)))
    probes = [tuple(p) for p in z["probes"]]
    pred_steps, goals, prev = [], [], None
    from peanut_amd.goal import GeodesicSolver
    st._goal = GeodesicSolver(st.full_w, st.full_h, int(args.col_rad), device=st.device)
    worst_probe = 0.0
    for i, fr in enumerate(frames):
        obs = torch.from_numpy(mapping_scenes.frame_to_obs(fr))[None].cuda()
        infos = {"sensor_pose": [float(v) for v in fr["pose"]], "goal_cat_id": int(z["goal_cat"])}
        if i == 0:
            st.init_with_obs(obs, infos)
        predicted = st.update_state(obs, infos)          # select_goal=False: goal selection is driven below, after the trail update
        cur = (int(st.loc_r + st.lmb[0]), int(st.loc_c + st.lmb[2]))
        goal_ref.mark_visited(vis, prev if prev is not None else cur, cur)
        prev = cur
        if predicted:
            st.visited_vis.copy_(torch.from_numpy(vis.astype(np.uint8)))
            k = len(pred_steps)
            res = st._goal.select(st.full_map[0], st.collision_map, st.visited_vis, st.lmb, (st.loc_r, st.loc_c), st.target_pred,
                                  500.0, int(args.map_resolution), want_dist=True)
            new = [res["goal"]]
            if new != st.last_global_goal:
                st.last_global_goal = st.global_goals
                st.global_goals = new
            pred_steps.append(i)
            goals.append([int(st.global_goals[0][0]), int(st.global_goals[0][1])])
            dd = res["dist"].cpu().numpy()
            ref_probe = z["dd_probe"][k]
            for p, rv in zip(probes, ref_probe):
                assert np.isinf(dd[p]) == np.isinf(rv), (i, p)
                if np.isfinite(rv):
                    worst_probe = max(worst_probe, abs(dd[p] - rv))
            assert int(np.isfinite(dd).sum()) == int(z["dd_reach"][k]), f"step {i}: reachable cells"
            assert abs(res["wt_sum"] - z["wt_sum"][k]) <= 1e-6 * max(1.0, z["wt_sum"][k]) + 0.5 or res["kept_last"]
            assert [int(v) for v in res["goal"]] == list(z["value_argmax"][k]), f"step {i}: argmax of the value map"
            last_dd = dd
    assert pred_steps == list(z["pred_steps"]), "prediction schedule (depends on the selected goals through dist_to_goal)"
    assert goals == [list(g) for g in z["global_goals"]]
    ref_last = z["last_dd_f32"].astype(np.float64)
    fin = ref_last >= 0
    assert np.array_equal(np.isfinite(last_dd), fin)
    err = np.abs(last_dd[fin] - ref_last[fin]).max()
    print(f"golden episode: goals {goals}; probes max |diff| {worst_probe:.2e}; last field max |diff| {err:.2e} (fp32-stored fixture)")
    assert worst_probe <= FIELD_TOL and err <= FIELD_TOL


def test_update_state_selects_goals_and_keeps_last_weights_when_stuck():
    """Agent_State.update_state with goal selection on (default): update_prediction -> update_global_goal; an agent
    walled in by obstacles (sum of weights < 10) keeps the previous weights (agent_state.py:398-399)."""
    from peanut_amd.goal import GeodesicSolver
    sol = GeodesicSolver(96, 96, 1)
    obst = torch.zeros((96, 96))           # no obstacle: every cell is reached, the farthest ones weigh 0 (:393)
    tp = torch.zeros((48, 48))
    tp[40, 40] = 1.0
    tp[3, 3] = 0.8
    lmb = (24, 72, 24, 72)
    r1, last = _select_and_check(sol, None, obst, None, None, lmb, (10, 10), tp, 500.0)
    assert not r1["kept_last"] and r1["wt_sum"] > 10
    v1 = r1["value"].cpu()
    obst2 = obst.clone()
    obst2[24 + 10 - 3:24 + 10 + 4, 24 + 10 - 3:24 + 10 + 4] = 1.0       # the agent's cell and its surroundings are blocked
    r2, last = _select_and_check(sol, last, obst2, None, None, lmb, (10, 10), tp, 500.0)
    assert r2["kept_last"] and r2["wt_sum"] < 10 and r2["goal"] == r1["goal"] and torch.equal(r2["value"].cpu(), v1)
    sol.reset()
    r3, last = _select_and_check(sol, None, obst2, None, None, lmb, (10, 10), tp, 500.0)
    assert not r3["kept_last"]                                            # nothing to fall back to after reset
    r4, last = _select_and_check(sol, last, obst, None, None, lmb, (10, 10), tp, -1.0)    # temperature -1: target_pred alone
    assert r4["goal"] == (40, 40)
    _select_and_check(sol, last, obst, None, None, lmb, (10, 10), None, 0.0)              # temperature 0: frontier mode


@pytest.mark.parametrize("shape,seed", [((960, 960), 1), ((480, 480), 2)], ids=lambda v: str(v))
def test_ordering_pass_cap_is_reported_and_its_effect_is_bounded(shape, seed):
    """The agent's map sizes (480 local, 960 full): under the DEFAULT ceiling (24, round 5) the ordering passes reach their fixed
    point and nothing is warned; a solve capped at six passes through the library option fmm_max_passes (the round-4 default)
    either reaches it too or says so (``converged`` False + ONE warning from the Python mirror), and the field it returns is
    within 0.1 cell of the fixed point -- the bound on what stopping early can cost FMMPlanner / goal selection."""
    import warnings
    from peanut_amd import _lib
    from peanut_amd.goal import GeodesicSolver
    h, w = shape
    trav = _maze(h, w, seed)
    src = (h // 2 + 3, w // 2 - 5)
    trav[src[0] - 2:src[0] + 3, src[1] - 2:src[1] + 3] = 1
    tt = torch.from_numpy(trav)
    with _lib.default_options(fmm_max_passes=6):
        sol = GeodesicSolver(h, w, 0)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            capped = sol.distance(tt, goal=src).cpu().numpy()
            capped_again = sol.distance(tt, goal=src).cpu().numpy()
    hit_cap = not sol.converged
    said = [r for r in rec if "ordering passes stopped at their cap" in str(r.message)]
    assert len(said) == (1 if hit_cap else 0), [str(r.message) for r in rec]
    assert np.array_equal(capped, capped_again)
    with warnings.catch_warnings(record=True) as rec2:
        warnings.simplefilter("always")
        free = GeodesicSolver(h, w, 0)                   # default options
        full = free.distance(tt, goal=src).cpu().numpy()
    assert free.converged and free.passes < 24, f"{free.passes} passes without reaching the ordering fixed point"
    assert not [r for r in rec2 if "ordering passes" in str(r.message)], "the default solve must run warning-free"
    fin = np.isfinite(full)
    assert np.array_equal(fin, np.isfinite(capped))
    diff = np.abs(full[fin] - capped[fin]).max()
    print(f"{h}x{w}: cap of six {'hit' if hit_cap else 'not hit'} ({sol.passes} passes), default: fixed point after {free.passes} passes; "
          f"capped vs fixed point max {diff:.3e} cells")
    assert diff <= 0.1


def test_field_solved_next_to_the_prediction_forward_is_the_same_field():
    """peanut_goal_select_begin (round 5): the field of a begun select runs on the handle's own stream, beside the work the
    caller enqueued after the begin (here a chain of large matrix products that ends in target_pred).  Same field, bit for bit,
    same goal, as the select alone; a select whose inputs differ from the begun ones ignores the begun work and solves its own."""
    from peanut_amd.goal import GeodesicSolver
    H = W = 480
    trav = _maze(H, W, 7)
    obst = torch.from_numpy((~trav.astype(bool)).astype(np.float32)).cuda()
    col = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    vis = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    lmb = (120, 360, 120, 360)
    g = torch.Generator().manual_seed(5)
    base = torch.rand((240, 240), generator=g).cuda()
    a = torch.rand((2048, 2048), generator=g).cuda()

    def produce_target():            # a few milliseconds of device work on the caller's stream
        x = a
        for _ in range(6):
            x = (x @ a) * (1.0 / 1024.0)
        return base + x[:240, :240] * 1e-9

    free = np.argwhere(trav[130:350, 130:350])[0] + 10
    loc = (int(free[0]), int(free[1]))
    sol = GeodesicSolver(H, W, 1)
    ref = sol.select(obst, col, vis, lmb, loc, produce_target(), 500.0, 5, want_dist=True, want_value=True)
    sol2 = GeodesicSolver(H, W, 1)
    for rep in range(3):             # (also with the round hints of a previous solve in place)
        sol2.reset()
        sol2.select_begin(obst, col, vis, lmb, loc)
        got = sol2.select(obst, col, vis, lmb, loc, produce_target(), 500.0, 5, want_dist=True, want_value=True)
        assert got["goal"] == ref["goal"] and got["wt_sum"] == ref["wt_sum"] and got["rounds"] >= 1      # (the sum is reduced in a fixed order)
        assert torch.equal(got["dist"], ref["dist"]) and torch.equal(got["value"], ref["value"])
    # an input that has to be converted (bool -> uint8) is converted once, at the begin, and the select reuses the buffer
    sol2.reset()
    cb = col.bool()
    sol2.select_begin(obst, cb, vis, lmb, loc)
    got = sol2.select(obst, cb, vis, lmb, loc, produce_target(), 500.0, 5, want_dist=True)
    assert got["goal"] == ref["goal"] and torch.equal(got["dist"], ref["dist"])
    # the agent's own call shape (agent_state.py: full_map[0] is a FRESH VIEW OBJECT on every call) with a bool collision map: the
    # begun inputs are recognised by their storage, so the select takes the begun field (begun_matches counts it) -- round 5 compared
    # object identities and silently re-solved serially here
    full_map = torch.stack([obst, obst * 0])
    sol2.reset()
    n0 = sol2.begun_matches
    sol2.select_begin(full_map[0], cb, vis, lmb, loc)
    got = sol2.select(full_map[0], col.bool(), vis, lmb, loc, produce_target(), 500.0, 5, want_dist=True)
    assert sol2.begun_matches == n0                       # a different (equal-valued) bool tensor is different storage: not matched
    assert got["goal"] == ref["goal"] and torch.equal(got["dist"], ref["dist"])
    sol2.reset()
    sol2.select_begin(full_map[0], cb, vis, lmb, loc)
    got = sol2.select(full_map[0], cb, vis, lmb, loc, produce_target(), 500.0, 5, want_dist=True)
    assert sol2.begun_matches == n0 + 1
    assert got["goal"] == ref["goal"] and torch.equal(got["dist"], ref["dist"])
    # a select for another agent cell than the one begun: the begun work is dropped, the answer is that of a select alone
    other = (loc[0] + 7, loc[1] + 3)
    alone = sol.select(obst, col, vis, lmb, other, produce_target(), 500.0, 5, want_dist=True)
    sol2.select_begin(obst, col, vis, lmb, loc)
    got = sol2.select(obst, col, vis, lmb, other, produce_target(), 500.0, 5, want_dist=True)
    assert got["goal"] == alone["goal"] and torch.equal(got["dist"], alone["dist"])
    # ... and a begin that no select follows does not disturb a distance transform on the same handle
    sol2.select_begin(obst, col, vis, lmb, loc)
    t_u8 = torch.from_numpy(trav).cuda()
    assert torch.equal(sol2.distance(t_u8, goal=(130, 140)), sol.distance(t_u8, goal=(130, 140)))


def test_update_state_with_and_without_the_overlapped_field_agree():
    """Agent_State.update_state marks the goal solver's inputs before the prediction forward (goal_overlap, default on): the
    episode's goals, prediction schedule and final map equal those of the serial order, and the overlap is taken on every
    prediction step (``begun_matches``)."""
    from oracle import mapping_scenes
    from oracle.agent_ref import agent_args, fake_pattern
    from peanut_amd.agent_state import Agent_State
    runs = []
    for overlap in (True, False):
        args = agent_args(dist_weight_temperature=500, select_goal=True, goal_overlap=overlap)
        st = Agent_State(args, prediction_model=FakePredictionGPU(fake_pattern(size=args.prediction_window)))
        frames = mapping_scenes.make_sequence(seed=11, n_frames=24)
        st.reset()
        goals, steps = [], []
        for i, fr in enumerate(frames):
            obs = torch.from_numpy(mapping_scenes.frame_to_obs(fr))[None].cuda()
            infos = {"sensor_pose": [float(v) for v in fr["pose"]], "goal_cat_id": 2}
            if i == 0:
                st.init_with_obs(obs, infos)
            if st.update_state(obs, infos):
                steps.append(i)
                goals.append(tuple(st.global_goals[0]))
                # every prediction step's select takes over the field its select_begin started (none without the overlap)
                assert st._goal.begun_matches == (len(steps) if overlap else 0), (overlap, i)
        runs.append((steps, goals, st.full_map.clone(), st.value_max))
    assert len(runs[0][0]) >= 2
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1] and runs[0][3] == runs[1][3]
    assert torch.equal(runs[0][2], runs[1][2])


@pytest.mark.parametrize("precision", ["fp32", "fp16x3"])
def test_real_prediction_forward_next_to_the_goal_field_is_bit_identical(precision):
    """The agent's own pair (agent_state.py:345-373 then :376-415) with the REAL prediction model: the goal solver's field runs on its own
    stream next to the 720 x 720 forward (peanut_goal_select_begin), whose smaller kernels leave LDS and registers for the solver's
    workgroups -- the two really share CUs.  Round 6 met one pair of kernels that did not survive such sharing (profiles/r9i), so this is
    held directly: the predicted target map, the goals and the final map of an episode equal those of the serial order bit for bit, in
    the fp32 mode and in an emulated mode."""
    from oracle import mapping_scenes
    from oracle.agent_ref import agent_args
    from peanut_amd.agent_state import Agent_State
    from peanut_amd.weights import PredCfg, make_seeded_state_dict
    sd = make_seeded_state_dict(PredCfg(), 0)
    runs = []
    for overlap in (True, False):
        args = agent_args(dist_weight_temperature=500, select_goal=True, goal_overlap=overlap, pred_precision=precision, only_explore=0)
        st = Agent_State(args, state_dict=sd)
        frames = mapping_scenes.make_sequence(seed=11, n_frames=24)
        st.reset()
        goals, preds = [], []
        for i, fr in enumerate(frames):
            obs = torch.from_numpy(mapping_scenes.frame_to_obs(fr))[None].cuda()
            infos = {"sensor_pose": [float(v) for v in fr["pose"]], "goal_cat_id": 2}
            if i == 0:
                st.init_with_obs(obs, infos)
            if st.update_state(obs, infos):
                goals.append(tuple(st.global_goals[0]))
                preds.append(st.target_pred.clone())
        runs.append((goals, preds, st.full_map.clone()))
        del st
    assert len(runs[0][0]) >= 2 and runs[0][0] == runs[1][0]
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    assert torch.equal(runs[0][2], runs[1][2])


def _obstacles(h, w, seed):
    """A full_map[0]-like obstacle map (values around the rint threshold) with the maze's walls."""
    rng = np.random.RandomState(seed)
    obst = (~_maze(h, w, seed).astype(bool)).astype(np.float32) * rng.choice([0.51, 1.0, 2.0], size=(h, w)).astype(np.float32)
    obst += (rng.rand(h, w) < 0.01).astype(np.float32) * 0.49          # below the threshold: free
    return torch.from_numpy(obst)


@pytest.mark.parametrize("temperature", [500.0, 1.0, -1.0, 0.0])
def test_selection_matches_the_restatement_on_the_device_field(temperature):
    """update_global_goal from the field onward, against oracle/goal_ref.select_from_field on the device's own field, over one
    episode-like sequence of calls per temperature (500; 1: the weights underflow, the stuck rule keeps the last ones; -1: target_pred
    alone; 0: frontier mode): a non-square full map and window, windows touching each border of the map, agent cells outside the map
    (np.clip), a map without obstacles (every cell reached: the farthest cells weigh 0), NaN in target_pred, and a reset."""
    from peanut_amd.goal import GeodesicSolver
    H, W = 200, 264
    sol = GeodesicSolver(H, W, 2)
    g = torch.Generator().manual_seed(int(temperature) + 7)
    obst = _obstacles(H, W, 11)
    col = torch.zeros((H, W), dtype=torch.uint8)
    col[100, 40:60] = 1
    vis = torch.zeros((H, W), dtype=torch.uint8)
    vis[60:70, 100:140] = 1
    empty = torch.zeros((H, W))
    calls = [  # (obstacles, lmb = (gx1, gx2, gy1, gy2), agent cell in the window)
        (obst, (50, 150, 70, 190), (50, 60)),         # inside, 100 x 120
        (obst, (0, 100, 70, 190), (30, 20)),          # top border
        (obst, (100, 200, 70, 190), (80, 100)),       # bottom border
        (obst, (50, 150, 0, 120), (-70, 50)),         # left border; agent above the map (clipped)
        (obst, (50, 150, 144, 264), (40, 200)),       # right border; agent right of the map (clipped)
        (empty, (50, 150, 70, 190), (50, 60)),        # no obstacles
        (empty, (100, 200, 144, 264), (-300, -300)),  # ... agent clipped to (0, 0): the map's farthest cell is in the window
        ("nan", (50, 150, 70, 190), (50, 60)),        # one NaN in target_pred
        ("reset", None, None),
        (obst, (0, 200, 0, 264), (100, 130)),         # the whole map as the window
        (obst, (30, 90, 10, 250), (20, 100)),         # 60 x 240
    ]
    last = None
    for k, (ob, lmb, loc) in enumerate(calls):
        if isinstance(ob, str) and ob == "reset":
            sol.reset()
            last = None
            continue
        tp = torch.rand((lmb[1] - lmb[0], lmb[3] - lmb[2]), generator=g)
        if isinstance(ob, str):
            ob = obst
            tp[37, 61] = float("nan")
        plain = ob is empty                            # no obstacle, no collision: no masked cell at all
        got, last = _select_and_check(sol, last, ob.cuda(), None if plain else col.cuda(), None if plain else vis.cuda(), lmb, loc,
                                      tp.cuda(), temperature)
        if isinstance(calls[k][0], str) and temperature != 0:
            assert got["goal"] == (37, 61), "np.argmax: the first NaN"
        if ob is empty:
            assert np.isfinite(got["dist"].cpu().numpy()).all()
            if lmb[0] == 100 and temperature in (500.0, 0.0):
                assert got["value"][-1, -1].item() == 0.0 and got["value"][-2, -1].item() > 0.0, "the farthest cell weighs 0 (:393)"

        if temperature == 1.0 and k in (1, 2, 3, 4, 5, 6):
            assert got["kept_last"], "temperature 1: the weights underflow and the last ones are kept"


@pytest.mark.parametrize("temperature", [-1.0, 500.0])
def test_argmax_plateaus_and_nan_over_a_window_of_many_workgroups(temperature):
    """A window larger than 256 x 1024 cells (the argmax's grid strides over it): an all-zero target_pred, equal maxima handled by
    different workgroups and by one lane in consecutive strides (temperature -1: exact ties, the first index wins), one NaN, and
    all NaN -- the goal is then the first cell, never a cell outside the window."""
    from peanut_amd.goal import GeodesicSolver
    H, W = 560, 600
    sol = GeodesicSolver(H, W, 1)
    obst = torch.zeros((H, W), device="cuda")
    obst[200:202, 100:500] = 1.0
    lmb = (10, 550, 40, 540)                        # 540 x 500 = 270000 cells > 262144
    lw, lh = lmb[1] - lmb[0], lmb[3] - lmb[2]
    loc = (300, 250)
    last = None
    tp = torch.zeros((lw, lh))
    got, last = _select_and_check(sol, last, obst, None, None, lmb, loc, tp.cuda(), temperature)
    # (workgroup, lane) of an index: ((i % 262144) // 256, i % 256); the first index, 300, is workgroup 1's, another maximum
    # sits in workgroup 0's second stride, one in a later workgroup, and one behind 300 in the same lane's next stride
    tp.view(-1)[[262144 + 10, 5000, 300, 262144 + 300]] = 0.75
    got, last = _select_and_check(sol, last, obst, None, None, lmb, loc, tp.cuda(), temperature)
    if temperature == -1.0:
        assert got["goal"] == divmod(300, lh)
    one = torch.rand((lw, lh), generator=torch.Generator().manual_seed(2))
    one.view(-1)[262144 + 77] = float("nan")
    one.view(-1)[200000] = float("nan")
    got, last = _select_and_check(sol, last, obst, None, None, lmb, loc, one.cuda(), temperature)
    assert got["goal"] == divmod(200000, lh)
    alln = torch.full((lw, lh), float("nan"))
    got, last = _select_and_check(sol, last, obst, None, None, lmb, loc, alln.cuda(), temperature)
    assert got["goal"] == (0, 0) and np.isnan(got["value_max"])


FIXED_POINT_GATE = 1.5e-6    # cells: stage B's 1e-6-cell noise threshold + the single-precision solve; measured maximum 1.25e-6


@pytest.mark.parametrize("shape,seed", [((960, 960), 21), ((480, 480), 22), ((250, 333), 23), ((31, 33), 24), ((7, 300), 25)],
                         ids=lambda v: str(v))
def test_fmm_field_is_the_fixed_point_of_its_scheme(shape, seed):
    """The returned field IS the fixed point of the scheme goal.hip solves, not merely within 0.5 cell of the heap-ordered march:
    one float64 stage-B update of every cell on the graph ordered by the field itself (oracle/goal_ref.fmm_fixed_point_residual)
    moves no reached cell by more than the gate, and the reached cells are exactly the 4-connected components of the traversible
    map that hold a seed.  One seed, and a goal mask with several seeds (one on a masked cell)."""
    from scipy import ndimage as ndi
    from oracle import goal_ref
    from peanut_amd.goal import GeodesicSolver
    h, w = shape
    trav = _maze(h, w, seed)
    rng = np.random.RandomState(seed)
    src = (h // 2, w // 2 - 1)
    trav[max(src[0] - 2, 0):src[0] + 3, max(src[1] - 2, 0):src[1] + 3] = 1
    gm = np.zeros((h, w), np.uint8)
    gm[rng.randint(0, h, 4), rng.randint(0, w, 4)] = 1
    gm[src] = 0
    ys, xs = np.nonzero(gm)
    trav[ys[0], xs[0]] = 0                              # a goal on a masked cell
    sol = GeodesicSolver(h, w, 0)
    worst = 0.0
    for goal, mask in ((src, None), (None, gm)):
        u = sol.distance(torch.from_numpy(trav), goal=goal, goal_mask=None if mask is None else torch.from_numpy(mask)).cpu().numpy()
        assert sol.converged
        seeds = np.zeros((h, w), bool)
        if mask is None:
            seeds[goal] = True
        else:
            seeds |= mask == 1
        labels, _ = ndi.label((trav != 0) | seeds)      # (default structure: 4-connected)
        reach = np.isin(labels, np.unique(labels[seeds]))
        assert np.array_equal(np.isfinite(u), reach), "reached cells = the seeds' components"
        assert (u[seeds] == 0).all()
        res, _ = goal_ref.fmm_fixed_point_residual(u, trav, seeds)
        worst = max(worst, float(res.max()))
        print(f"{h}x{w} {'goal cell' if mask is None else 'goal mask'}: fixed-point residual max {res.max():.3e} cells "
              f"over {int(reach.sum())} reached cells ({sol.passes} ordering passes)")
    assert worst <= FIXED_POINT_GATE


def test_select_begin_on_reused_storage_or_edited_inputs_solves_the_new_inputs():
    """select_begin recognises the select that continues its work by the inputs' storage.  A temporary input (collision.bool())
    whose block the allocator could hand to the next temporary, and an input written in place between the two calls, must not
    make the select reuse the begun field: the result equals that of a select alone (the test says whether the allocator reused
    the block)."""
    from peanut_amd.goal import GeodesicSolver
    H = W = 240
    obst = _obstacles(H, W, 31).cuda()
    lmb, loc = (40, 200, 40, 200), (80, 80)
    obst[40 + 70:40 + 90, 40 + 70:40 + 90] = 0.0        # the agent's surroundings are free
    col_a = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    col_b = col_a.clone()
    col_b[40 + 60:40 + 100, 40 + 90] = 1                 # a wall next to the agent: another field
    vis = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    tp = torch.rand((160, 160), generator=torch.Generator().manual_seed(3)).cuda()
    alone = GeodesicSolver(H, W, 1)
    sol = GeodesicSolver(H, W, 1)

    def begin_on_a_temporary():
        t = col_a.bool()
        sol.select_begin(obst, t, vis, lmb, loc)
        return t.data_ptr()

    ptr_a = begin_on_a_temporary()
    tb = col_b.bool()
    reused = tb.data_ptr() == ptr_a
    got = sol.select(obst, tb, vis, lmb, loc, tp, 500.0, 5, want_dist=True, want_value=True)
    ref = alone.select(obst, tb, vis, lmb, loc, tp, 500.0, 5, want_dist=True, want_value=True)
    print(f"allocator handed the begun temporary's block to the next one: {reused}")
    assert torch.equal(got["dist"], ref["dist"]) and got["goal"] == ref["goal"] and got["wt_sum"] == ref["wt_sum"]
    # written in place between select_begin and select (obstacles and collision map already in the library's formats)
    obst2, col2 = obst.clone(), col_a.clone()
    sol.reset()
    alone.reset()
    sol.select_begin(obst2, col2, vis, lmb, loc)
    obst2[40 + 60:40 + 100, 40 + 70] = 1.0
    got = sol.select(obst2, col2, vis, lmb, loc, tp, 500.0, 5, want_dist=True)
    ref = alone.select(obst2, col2, vis, lmb, loc, tp, 500.0, 5, want_dist=True)
    assert torch.equal(got["dist"], ref["dist"]) and got["goal"] == ref["goal"]
    # ... through a view of a larger map (Agent_State passes full_map[0]): the view shares the map's version counter
    full = torch.stack([obst, obst * 0])
    sol.select_begin(full[0], col2, vis, lmb, loc)
    full[0, 40 + 75, 40 + 60:40 + 100] = 1.0
    got = sol.select(full[0], col2, vis, lmb, loc, tp, 500.0, 5, want_dist=True)
    ref = alone.select(full[0], col2, vis, lmb, loc, tp, 500.0, 5, want_dist=True)
    assert torch.equal(got["dist"], ref["dist"]) and got["goal"] == ref["goal"]
    n0 = sol.begun_matches
    sol.select_begin(full[0], col2, vis, lmb, loc)          # unchanged inputs: the begun field is taken over
    got = sol.select(full[0], col2, vis, lmb, loc, tp, 500.0, 5, want_dist=True)
    assert sol.begun_matches == n0 + 1 and torch.equal(got["dist"], ref["dist"])


def test_selection_is_deterministic():
    """Repeated selects on the same inputs: the same sum of weights, value map and goal, bit for bit (the sum decides the
    keep-last rule, so it must not vary in its last digits)."""
    from peanut_amd.goal import GeodesicSolver
    H = W = 960
    obst = _obstacles(H, W, 41).cuda()
    obst[470:490, 470:490] = 0.0
    tp = torch.rand((960, 960), generator=torch.Generator().manual_seed(4)).cuda()
    sol = GeodesicSolver(H, W, 1)
    first = None
    for _ in range(6):
        sol.reset()
        got = sol.select(obst, None, None, (0, 960, 0, 960), (480, 480), tp, 500.0, 5, want_value=True)
        key = (got["goal"], np.float64(got["wt_sum"]).tobytes(), np.float64(got["value_max"]).tobytes())
        if first is None:
            first, v0 = key, got["value"]
        assert key == first
        assert torch.equal(got["value"], v0)


# ---- the solver's other kernels: options fmm_blocked, fmm_local32, fmm_inner ----
# enqueue_rounds (csrc/goal.hip) launches one of four instantiations per stage: fmm_round_blocked_kernel or fmm_round_kernel,
# each with the single-precision or the float64 local solve.  Everything above runs (blocked, local32) = (1, 1) with 48 inner
# iterations; here every pair runs, and the blocked kernels also with 1 and 1024 inner iterations (the ends of the option's range).
FMM_VARIANTS = [(1, 1, 48), (1, 1, 1), (1, 1, 1024), (1, 0, 48), (1, 0, 1), (1, 0, 1024), (0, 1, 48), (0, 0, 48)]
VARIANT_SHAPES = [((250, 333), 23), ((64, 40), 4), ((31, 33), 24), ((7, 300), 25)]


def _variant_solver(h, w, blocked, local32, inner):
    from peanut_amd import _lib
    from peanut_amd.goal import GeodesicSolver
    with _lib.default_options(fmm_blocked=blocked, fmm_local32=local32, fmm_inner=inner):
        return GeodesicSolver(h, w, 0)


def _variant_solve(sol, trav, src, gm):
    """-> [(field, rounds, passes)] of the two solves: one goal cell, a goal mask of several seeds."""
    out = []
    for goal, mask in ((src, None), (None, gm)):
        u = sol.distance(torch.from_numpy(trav), goal=goal, goal_mask=None if mask is None else torch.from_numpy(mask)).cpu().numpy()
        assert sol.converged
        out.append((u, sol.rounds, sol.passes))
    return out


@pytest.fixture(scope="module")
def variant_cases():
    """shape -> (map, goal cell, goal mask, seed sets of the two solves, their oracle fields, the default solver's two solves): made
    once for the module, before any variant runs, and read-only from then on."""
    cases = {}
    for shape, seed in VARIANT_SHAPES:
        h, w = shape
        trav = _maze(h, w, seed)
        rng = np.random.RandomState(seed)
        src = (h // 2, w // 2 - 1)
        trav[max(src[0] - 2, 0):src[0] + 3, max(src[1] - 2, 0):src[1] + 3] = 1
        gm = np.zeros((h, w), np.uint8)
        gm[rng.randint(0, h, 4), rng.randint(0, w, 4)] = 1
        gm[src] = 0
        ys, xs = np.nonzero(gm)
        trav[ys[0], xs[0]] = 0                              # a goal on a masked cell
        seeds = [np.zeros((h, w), bool), gm == 1]
        seeds[0][src] = True
        refs = [_oracle_field(trav, list(zip(*np.nonzero(s)))) for s in seeds]
        base = _variant_solve(_variant_solver(h, w, 1, 1, 48), trav, src, gm)
        for a in [trav, gm] + seeds + refs + [u for u, _, _ in base]:
            a.setflags(write=False)
        cases[shape] = (trav, src, gm, seeds, refs, base)
    return cases


@pytest.mark.parametrize("blocked,local32,inner", FMM_VARIANTS, ids=lambda v: str(v))
@pytest.mark.parametrize("shape", [s for s, _ in VARIANT_SHAPES], ids=lambda v: "x".join(map(str, v)))
def test_fmm_solver_variants_meet_the_gates_of_the_default(variant_cases, shape, blocked, local32, inner):
    """Every (fmm_blocked, fmm_local32) instantiation of the relaxation round, and fmm_inner = 1 / 48 / 1024 on the blocked ones, on
    maps whose tile edges are ragged (32 x 32 tiles: 250 x 333, 64 x 40, 31 x 33, 7 x 300): the field within FIELD_TOL of the
    heap-ordered oracle, the fixed point of its own scheme to FIXED_POINT_GATE, and finite on exactly the cells the oracle reaches
    and the seeds' 4-connected components hold -- one goal cell and a goal mask with a seed on a masked cell.

    Which kernel ran shows in the solve itself, on the 250 x 333 map's goal-cell field: the whole-tile sweep (fmm_blocked = 0), one
    inner iteration per round (fmm_inner = 1) and the float64 local solve (fmm_local32 = 0) each return a field that differs from the
    default's in the last bits of most cells (another schedule lands elsewhere inside stage B's noise threshold), and the float64 solve
    sits at its own fixed point to 1e-8 cell -- out of reach of an increment computed in single precision (2^-24 of a step of about
    one cell is 6e-8).  The number of rounds is printed, not asserted: the sweep needs exactly the default's 44 here.  fmm_inner = 1024
    only lets a wave iterate longer before it publishes its block; on these maps a block has converged long before, the field equals
    the default's bit for bit (asserted), and the case holds that setting to the same gates: the option only reschedules.

    fmm_local32 = 0: its distance to the oracle is printed next to the default's and must not be larger (up to the oracle's own
    float64 rounding, 1e-9 cell)."""
    from scipy import ndimage as ndi
    from oracle import goal_ref
    h, w = shape
    trav, src, gm, seeds, refs, base = variant_cases[shape]
    got = _variant_solve(_variant_solver(h, w, blocked, local32, inner), trav.copy(), src, gm.copy())
    for k, ((u, rounds, passes), (u0, rounds0, passes0), ref, sd) in enumerate(zip(got, base, refs, seeds)):
        what = f"{h}x{w} blocked={blocked} local32={local32} inner={inner} {'goal cell' if k == 0 else 'goal mask'}"
        labels, _ = ndi.label((trav != 0) | sd)
        reach = np.isin(labels, np.unique(labels[sd]))
        assert np.array_equal(np.isfinite(u), reach), f"{what}: reached cells = the seeds' components"
        assert np.array_equal(np.isinf(u), np.isinf(ref)) and np.array_equal(np.isinf(u), np.isinf(u0)), f"{what}: reached cells"
        assert (u[sd] == 0).all()
        fin = np.isfinite(ref)
        err, err0 = float(np.abs(u[fin] - ref[fin]).max()), float(np.abs(u0[fin] - ref[fin]).max())
        res, _ = goal_ref.fmm_fixed_point_residual(u, trav, sd)
        print(f"{what}: max |GPU - oracle| {err:.3e} cells (default solver {err0:.3e}), fixed-point residual {float(res.max()):.3e}, "
              f"{rounds} rounds in {passes} passes (default {rounds0} in {passes0}), "
              f"{int((u[fin] != u0[fin]).sum())} of {int(fin.sum())} cells differ from the default's in some bit")
        assert err <= FIELD_TOL, what
        assert float(res.max()) <= FIXED_POINT_GATE, what
        if not local32:
            assert err <= err0 + 1e-9, f"{what}: the float64 local solve is further from the oracle than the single-precision one"
        if shape == (250, 333) and k == 0:
            differs = int((u[fin] != u0[fin]).sum())
            if not local32:
                assert differs > 0, f"{what}: the float64 local solve returned the single-precision field"
                assert float(res.max()) <= 1e-8, f"{what}: a fixed-point residual of {float(res.max()):.3e} is no float64 local solve"
            elif not blocked or inner == 1:
                assert differs > 0, f"{what}: the default kernel's field, bit for bit"
            else:
                assert differs == 0, f"{what}: {differs} cells differ from the default's"
