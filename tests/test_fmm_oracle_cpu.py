"""The scikit-fmm restatement (oracle/fmm_ref.c; PARITY UNPINNED -- scikit-fmm itself is absent) against what IS
published about `skfmm.distance`: the docstring example of scikit-fmm's `distance` (3x3, phi = 1 with a -1 centre),
plus properties of the eikonal solution, and the goal-selection restatement (oracle/goal_ref.py) against the golden
episode produced by the reference's own Agent_State.update_global_goal (oracle/gen_golden_goal.py)."""
import os

import numpy as np
from numpy import ma

from oracle import fmm_ref, goal_ref


def test_skfmm_docstring_example():
    """scikit-fmm, skfmm/pfmm.py, docstring of distance():
        >>> phi = np.ones((3, 3)); phi[1, 1] = -1
        >>> skfmm.distance(phi)
        array([[ 1.20710678,  0.5       ,  1.20710678],
               [ 0.5       , -0.35355339,  0.5       ],
               [ 1.20710678,  0.5       ,  1.20710678]])"""
    phi = np.ones((3, 3))
    phi[1, 1] = -1
    want = np.array([[1.20710678, 0.5, 1.20710678], [0.5, -0.35355339, 0.5], [1.20710678, 0.5, 1.20710678]])
    np.testing.assert_allclose(fmm_ref.distance(phi), want, atol=5e-9)


def test_point_source_free_space():
    t = ma.masked_values(np.ones((161, 161)), 0)
    t[80, 80] = 0
    d = fmm_ref.distance(t, dx=1)
    yy, xx = np.mgrid[:161, :161]
    e = np.hypot(yy - 80, xx - 80)
    assert not ma.is_masked(d)
    assert np.abs(d[80, 80:100] - np.arange(20.0)).max() < 1e-9      # along the axes the scheme is exact
    assert np.abs(d - e).max() < 0.35                              # second order: well under half a cell
    assert np.abs(fmm_ref.distance(t, dx=1, order=1) - e).max() > 1.0
    assert np.allclose(d, d.T) and np.allclose(d, d[::-1]) and np.allclose(d, d[:, ::-1])


def test_masked_corridor_and_unreachable_pocket():
    trav = np.zeros((40, 60))
    trav[5, 5:50] = 1          # corridor east ...
    trav[5:30, 49] = 1         # ... then south
    trav[35:38, 10:20] = 1     # pocket the front cannot reach
    t = ma.masked_values(trav * 1, 0)
    t[5, 5] = 0
    d = fmm_ref.distance(t, dx=1)
    assert abs(d[5, 49] - 44.0) < 1e-9 and abs(d[29, 49] - 68.0) < 1e-9    # path length around the corner
    m = ma.getmaskarray(d)
    assert m[36, 15] and m[0, 0] and not m[5, 30]                  # unreached / masked cells come back masked
    filled = goal_ref.fmm_set_goal(trav, (5, 5))
    assert abs(filled[36, 15] - 69.0) < 1e-9 and filled[0, 0] == filled[36, 15]      # ma.filled(dd, max + 1)
    gm = np.zeros_like(trav)
    gm[5, 5] = gm[29, 49] = 1
    d2 = goal_ref.fmm_set_multi_goal(trav, gm)
    assert abs(d2[5, 49] - 24.0) < 1e-9 and abs(d2[5, 27] - 22.0) < 1e-9


def test_goal_restatement_matches_reference_golden(golden_dir):
    """oracle/goal_ref.GoalSelector replays the golden episode's goal sequence given the recorded distance field of
    the last prediction step (the full episode replay is the GPU test's job; here: the weighting / argmax / 'avoid the
    last goal' bookkeeping on a synthetic value map)."""
    z = np.load(os.path.join(golden_dir, "goal_golden.npz"))
    assert list(z["pred_steps"]) == sorted(z["pred_steps"]) and len(z["global_goals"]) == len(z["pred_steps"])
    dd = z["last_dd_f32"].astype(np.float64)
    assert (dd >= 0).sum() == int(z["dd_reach"][-1])
    from types import SimpleNamespace
    sel = goal_ref.GoalSelector(SimpleNamespace(col_rad=4, dist_weight_temperature=500, map_resolution=5), (64, 64))
    obst = np.zeros((64, 64), np.float32)
    obst[20:44, 30] = 1.0                                          # a wall between the agent and the better target
    tp = np.zeros((32, 32))
    tp[5, 28] = 1.0                                                # beyond the wall: far geodesically
    tp[28, 4] = 0.9                                                # same side as the agent
    zero = np.zeros((64, 64))
    g = sel.update(obst, (16, 48, 16, 48), (16, 2), tp, zero, zero)
    assert [tuple(int(v) for v in x) for x in g] == [(5, 28)] or [tuple(int(v) for v in x) for x in g] == [(28, 4)]
    w_far, w_near = sel.dd_wt[5, 28], sel.dd_wt[28, 4]
    assert (w_far * 1.0 > w_near * 0.9) == (tuple(int(v) for v in g[0]) == (5, 28))
    g2 = sel.update(obst, (16, 48, 16, 48), (16, 2), tp, zero, zero)          # same argmax again: goal list unchanged
    assert g2 == g


def test_adjacent_equal_seeds_use_the_second_order_term():
    """updatePointOrderTwo admits the second upwind neighbour when it is NOT FARTHER than the first (`<=`): next to two
    adjacent seeds the cell in line with them solves (9/4) u^2 = 1 -> 2/3, where a lone seed gives the first-order 1.
    (FMMPlanner.set_multi_goal's goal blobs, fmm_planner.py:67-75; the region feeds get_short_term_goal's stop test.)"""
    t = ma.masked_values(np.ones((9, 21)), 0)
    t[4, 9] = 0
    t[4, 10] = 0                                      # two seeds side by side in a row
    d = fmm_ref.distance(t, dx=1)
    assert d[4, 9] == 0 and d[4, 10] == 0
    assert abs(d[4, 11] - 2.0 / 3.0) < 1e-12 and abs(d[4, 8] - 2.0 / 3.0) < 1e-12     # in line with the pair
    assert abs(d[3, 9] - 1.0) < 1e-12 and abs(d[5, 10] - 1.0) < 1e-12                 # across the pair: one seed per axis
    lone = ma.masked_values(np.ones((9, 21)), 0)
    lone[4, 9] = 0
    dl = fmm_ref.distance(lone, dx=1)
    assert abs(dl[4, 10] - 1.0) < 1e-12 and abs(dl[4, 8] - 1.0) < 1e-12 and abs(dl[3, 9] - 1.0) < 1e-12
    # mirror symmetry about the pair (column c <-> 19 - c) holds to a few hundredths of a cell only: the j = -1 direction is
    # examined first and its value2 survives (the library's loop), and equal keys leave the heap in insertion order
    assert np.abs(d[:, 0:9] - d[:, 19:10:-1]).max() < 0.05


class _StatementSelector:
    """update_global_goal (agent_state.py:376-415) statement by statement, as oracle/goal_ref.GoalSelector.update read before it
    was routed through select_from_field: the yardstick that routing is held to."""

    def __init__(self, args, full_hw):
        from oracle.agent_ref import disk
        self.args, (self.full_w, self.full_h) = args, full_hw
        self.selem = disk(int(args.col_rad))
        self.dd_wt = None
        self.last_global_goal = None
        self.global_goals = None

    def update(self, full_obstacle, lmb, loc_rc, target_pred, collision_map, visited_vis):
        args = self.args
        trav = goal_ref.traversible_map(full_obstacle, self.selem, collision_map, visited_vis)
        r = int(np.clip(loc_rc[0] + lmb[0], 0, self.full_w - 1))
        c = int(np.clip(loc_rc[1] + lmb[2], 0, self.full_h - 1))
        traversible_ma = ma.masked_values(trav * 1, 0)
        traversible_ma[r, c] = 0
        dd = fmm_ref.distance(traversible_ma, dx=1)
        dd = ma.filled(dd, np.max(dd) + 1)
        dd[np.where(dd == np.max(dd))] = np.inf
        temperature = args.dist_weight_temperature / args.map_resolution
        with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
            dd_wt = np.exp(-dd / temperature)[lmb[0]:lmb[1], lmb[2]:lmb[3]]
            self.wt_sum = np.sum(dd_wt)
            if np.sum(dd_wt) < 10 and self.dd_wt is not None:
                dd_wt = self.dd_wt
            if args.dist_weight_temperature == -1:
                value = target_pred
            elif args.dist_weight_temperature == 0:
                dd = dd.copy()
                dd[np.where(dd < 60)] = np.inf
                value = np.exp(-dd / 100.)[lmb[0]:lmb[1], lmb[2]:lmb[3]]
            else:
                value = target_pred * dd_wt
        self.dd_wt = dd_wt
        self.value = value
        new_global_goal = [np.unravel_index(value.argmax(), value.shape)]
        if new_global_goal != self.last_global_goal:
            self.last_global_goal = self.global_goals
            self.global_goals = new_global_goal
        return self.global_goals


def _same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def test_select_from_field_reproduces_update_global_goal_in_every_mode():
    """oracle/goal_ref.select_from_field on the fmm_ref field reproduces the whole update_global_goal bit for bit -- value map,
    weights carried to the next call, their sum, goal list -- over call sequences in every temperature mode (500; 1, where the
    weights underflow and the stuck rule keeps the last ones; -1; 0), on a map with walls and on one without obstacles (every
    cell reached: the farthest cells become +inf), with agent cells that need the clip, NaN in target_pred, and a reset."""
    from types import SimpleNamespace
    rng = np.random.RandomState(3)
    H, W = 70, 90
    walls = np.zeros((H, W), np.float32)
    walls[10:50, 40] = 1.0
    walls[30, 5:35] = 1.0
    walls[55:60, 60:65] = 1.0
    lmb = (6, 66, 12, 84)
    zero = np.zeros((H, W))
    col = zero.copy()
    col[20, 20:30] = 1
    for temp in (500, 1, -1, 0):
        args = SimpleNamespace(col_rad=1, dist_weight_temperature=temp, map_resolution=5)
        new, old = goal_ref.GoalSelector(args, (H, W)), _StatementSelector(args, (H, W))
        calls = [(walls, (20, 10), col), (np.zeros_like(walls), (30, 40), zero), (walls, (-9, 80), zero),
                 (walls, (70, -20), col), ("reset", None, None), (walls, (25, 30), zero)]
        for k, (obst, loc, cm) in enumerate(calls):
            if isinstance(obst, str):
                new.reset()
                old.dd_wt, old.last_global_goal, old.global_goals = None, None, None
                continue
            tp = rng.rand(lmb[1] - lmb[0], lmb[3] - lmb[2]).astype(np.float32)
            if k == 2:
                tp[7, 9] = np.nan
            g_new = new.update(obst, lmb, loc, tp, cm, zero)
            g_old = old.update(obst, lmb, loc, tp, cm, zero)
            assert [tuple(int(v) for v in x) for x in g_new] == [tuple(int(v) for v in x) for x in g_old], (temp, k)
            assert _same_bits(new.value, old.value), (temp, k)
            assert _same_bits(new.dd_wt, old.dd_wt), (temp, k)
            assert _same_bits(new.wt_sum, old.wt_sum), (temp, k)
            if k == 2 and temp != 0:
                assert tuple(int(v) for v in g_new[0]) == (7, 9), "np.argmax: the first NaN wins"
            if k == 1 and temp == 500:
                assert np.isinf(new.dd).sum() >= 1 and np.isfinite(new.dd).sum() < H * W, "all reached: the farthest become +inf"
        if temp == 1:
            assert new.kept_last is False                   # (the last call follows a reset: nothing to keep)


def test_fixed_point_residual_restates_the_scheme():
    """oracle/goal_ref.fmm_fixed_point_residual: on open ground the heap-ordered march (fmm_ref) and the relaxation agree, so the
    march's own field is a fixed point of the restated update to the last bit (one seed, and several with two of them adjacent);
    moving one cell by 1e-4 shows up in the residual, and a free cell left unreached next to reached ones is updated."""
    trav = np.ones((40, 56), np.uint8)
    seeds = np.zeros(trav.shape, bool)
    seeds[13, 22] = True
    u = goal_ref.geodesic_field(trav, (13, 22))
    res, upd = goal_ref.fmm_fixed_point_residual(u, trav, seeds)
    assert res.max() == 0.0 and upd[13, 22] == 0.0
    bent = u.copy()
    bent[20, 30] += 1e-4
    assert goal_ref.fmm_fixed_point_residual(bent, trav, seeds)[0].max() >= 0.5e-4
    gm = np.zeros(trav.shape, bool)
    gm[5, 5] = gm[30, 50] = gm[31, 50] = True              # several seeds, two of them adjacent
    u2 = goal_ref.fmm_set_multi_goal(trav, gm)
    assert goal_ref.fmm_fixed_point_residual(u2, trav, gm)[0].max() <= 1e-12
    # a reached cell next to an unreached free one: the update reaches it (the unreached pattern is not a fixed point)
    holed = u.copy()
    holed[25, 10] = np.inf
    assert np.isfinite(goal_ref.fmm_fixed_point_residual(holed, trav, seeds)[1][25, 10])
