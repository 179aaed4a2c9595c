"""ORACLE (test infrastructure, not product code): CPU restatement of the long-term goal selection of the reference,
``Agent_State.update_global_goal`` (nav/agent/agent_state.py:376-415), and of ``FMMPlanner.set_goal /
set_multi_goal`` (nav/agent/utils/fmm_planner.py:55-75), in NumPy + scipy.ndimage + oracle/fmm_ref (the
scikit-fmm stand-in -- PARITY UNPINNED for that piece, see fmm_ref.c).

``skimage.morphology.binary_dilation(image, footprint)`` is ``scipy.ndimage.binary_dilation(image,
structure=footprint)`` (scikit-image's implementation is that one call; zero border)."""
from __future__ import annotations

import numpy as np
from numpy import ma
from scipy import ndimage as ndi

from oracle import fmm_ref
from oracle.agent_ref import disk


def binary_dilation(image, footprint=None):
    return ndi.binary_dilation(np.asarray(image) != 0, structure=footprint)


def mark_visited(visited_vis, prev_rc, cur_rc, half=2):
    """Test-harness stand-in for the trail Agent_Helper draws into ``visited_vis`` between consecutive agent cells
    (agent_helper.py:262-266, vu.draw_line): a (2*half+1)-wide bar of samples along the segment, full-map cells."""
    (r0, c0), (r1, c1) = prev_rc, cur_rc
    n = max(abs(r1 - r0), abs(c1 - c0), 1)
    H, W = visited_vis.shape
    for k in range(n + 1):
        r = int(round(r0 + (r1 - r0) * k / n))
        c = int(round(c0 + (c1 - c0) * k / n))
        visited_vis[max(r - half, 0):min(r + half + 1, H), max(c - half, 0):min(c + half + 1, W)] = 1
    return visited_vis


def traversible_map(full_obstacle, selem, collision_map, visited_vis):
    """agent_state.py:382-386."""
    trav = binary_dilation(np.rint(full_obstacle), selem) != True  # noqa: E712
    trav[collision_map == 1] = 0
    trav[visited_vis == 1] = 1
    return trav


def geodesic_field(trav, seed_rc):
    """agent_state.py:388-391: masked FMM from the agent's cell, as a plain array with +inf where the result is masked (masked or
    unreachable cells) -- the form of the field the device returns (``select(..., want_dist=True)``)."""
    traversible_ma = ma.masked_values(trav * 1, 0)
    traversible_ma[seed_rc[0], seed_rc[1]] = 0
    dd = fmm_ref.distance(traversible_ma, dx=1)
    return np.where(ma.getmaskarray(dd), np.inf, ma.getdata(dd))


def fill_field(dd_raw):
    """agent_state.py:392-393 on a field with +inf for its masked cells: ``ma.filled(dd, max + 1)``, then every cell equal to the
    maximum becomes +inf -- the filled cells when there are any, else the farthest reached cells."""
    dd = ma.masked_invalid(np.asarray(dd_raw, dtype=np.float64))
    dd = ma.filled(dd, np.max(dd) + 1)
    dd[np.where(dd == np.max(dd))] = np.inf
    return dd


def geodesic_distance(trav, seed_rc):
    """agent_state.py:388-393: masked FMM from the agent's cell; +inf where masked or unreachable."""
    return fill_field(geodesic_field(trav, seed_rc))


def select_from_field(dd_raw, lmb, target_pred, temperature, map_resolution, last_dd_wt):
    """update_global_goal from ``skfmm.distance`` onward (agent_state.py:392-413), in float64 NumPy: the field ``dd_raw`` [H,W]
    (+inf = masked / unreachable) -> fill and max -> inf, weights exp(-dd / (temperature / map_resolution)) over the window
    lmb = (gx1, gx2, gy1, gy2), the "sum < 10: keep the last weights" rule, the value map of the temperature's mode (-1: target_pred
    alone; 0: frontier weights exp(-dd'/100), dd' = inf below 60; else target_pred * weights) and its first-occurrence argmax.

    Returns (goal, value, wt_sum, kept_last, new_last): goal = the argmax cell (r, c) of the window, value [w,h], wt_sum = the sum
    of the fresh weights, kept_last = whether ``last_dd_wt`` replaced them, new_last = the weights carried to the next call
    (``self.dd_wt``).  At temperature 0 the weights are exp(-dd / 0) and are not used for the value."""
    gx1, gx2, gy1, gy2 = (int(v) for v in lmb)
    dd = fill_field(dd_raw)
    temperature_ = temperature / map_resolution
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        dd_wt = np.exp(-dd / temperature_)[gx1:gx2, gy1:gy2]
        wt_sum = float(np.sum(dd_wt))
    kept_last = bool(wt_sum < 10 and last_dd_wt is not None)
    if kept_last:                                       # stuck inside an obstacle: keep the last weights
        dd_wt = last_dd_wt
    with np.errstate(invalid="ignore"):
        if temperature == -1:
            value = np.asarray(target_pred)
        elif temperature == 0:
            dd = dd.copy()
            dd[np.where(dd < 60)] = np.inf
            value = np.exp(-dd / 100.)[gx1:gx2, gy1:gy2]
        else:
            value = target_pred * dd_wt
    goal = tuple(int(v) for v in np.unravel_index(value.argmax(), value.shape))
    return goal, value, wt_sum, kept_last, dd_wt


def _axis_pick(m1, m2, p1, p2):
    """One axis of the stage-B update (csrc/goal.hip axis_term): the nearer upwind neighbour v1 -- the j = -1 side unless the
    j = +1 side is strictly closer -- and the second neighbour BEHIND IT on the same side when it is not farther (<=)."""
    inf = np.inf
    v1 = np.where(m1 < inf, m1, inf)
    v2 = np.where((m1 < inf) & (m2 <= v1), m2, inf)
    plus = p1 < v1
    v2 = np.where(plus, np.where(p2 <= p1, p2, inf), v2)
    v1 = np.where(plus, p1, v1)
    return v1, v2


def _coeffs(v1, v2):
    """(a, b, c) of an axis: (9/4) (u - (4 v1 - v2) / 3)^2 with a second neighbour, (u - v1)^2 with one, nothing without."""
    aa = 9.0 / 4.0
    with np.errstate(invalid="ignore"):
        tp = (1.0 / 3.0) * (4.0 * v1 - v2)
        two = v2 < np.inf
        one = ~two & (v1 < np.inf)
        a = np.where(two, aa, np.where(one, 1.0, 0.0))
        b = np.where(two, -2.0 * aa * tp, np.where(one, -2.0 * v1, 0.0))
        c = np.where(two, aa * tp * tp, np.where(one, v1 * v1, 0.0))
    return a, b, c


def _root(a, b, c):
    """Larger root of a u^2 + b u + c = 1 (solveQuadratic for phi > 0); -1 without a real root."""
    c = c - 1.0
    det = b * b - 4.0 * a * c
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(det >= 0.0, (-b + np.sqrt(np.maximum(det, 0.0))) / 2.0 / a, -1.0)


def fmm_fixed_point_residual(u, trav, seeds):
    """How far the field ``u`` [H,W] (+inf = masked / unreached) is from the fixed point of the scheme csrc/goal.hip solves: one
    stage-B update of every cell, in float64, on the dependency graph ordered by ``u`` itself (ord = u, the last ordering pass of a
    converged solve).  A first neighbour feeds a cell when it is strictly earlier, a second one when it is not later than the first
    (fmm_round_blocked_kernel's feed predicates); masked cells (trav == 0, not a seed), cells outside the map and unreached cells
    never feed.  The update is that of oracle/fmm_ref.c (second-order term (9/4)(u - (4 v1 - v2)/3)^2, first-order (u - v1)^2,
    larger root), with the device's two documented departures from the heap-ordered march: the second neighbour belongs to v1's
    own side, and the second axis joins only when its neighbour lies below the one-axis root and the joint root stays above it
    (goal.hip, update_cell).

    Returns (residual, update): residual [H,W] = |u - update(u)| on every reached free non-seed cell, 0 elsewhere; update = the
    updated field (+inf where nothing feeds a free cell; the input value on seeds and masked cells)."""
    u = np.asarray(u, dtype=np.float64)
    trav = np.asarray(trav) != 0
    seeds = np.asarray(seeds) != 0
    H, W = u.shape
    inf = np.inf
    v = np.where(trav | seeds, u, inf)
    P = np.full((H + 4, W + 4), inf)
    P[2:-2, 2:-2] = v

    def at(dy, dx):
        return P[2 + dy:2 + dy + H, 2 + dx:2 + dx + W]

    def feeds(n1, n2):          # the neighbour pair (one step, two steps) as the cell sees it: +inf where it may not feed
        f1 = np.where(n1 < v, n1, inf)
        f2 = np.where(n2 <= n1, n2, inf)
        return f1, f2

    ym1, ym2 = feeds(at(-1, 0), at(-2, 0))
    yp1, yp2 = feeds(at(1, 0), at(2, 0))
    xm1, xm2 = feeds(at(0, -1), at(0, -2))
    xp1, xp2 = feeds(at(0, 1), at(0, 2))
    yv1, yv2 = _axis_pick(ym1, ym2, yp1, yp2)
    xv1, xv2 = _axis_pick(xm1, xm2, xp1, xp2)
    hy, hx = yv1 < inf, xv1 < inf
    y_first = hy & (~hx | (yv1 <= xv1))
    s1, s2 = np.where(y_first, yv1, xv1), np.where(y_first, yv2, xv2)
    o1, o2 = np.where(y_first, xv1, yv1), np.where(y_first, xv2, yv2)
    sa, sb, sc = _coeffs(s1, s2)
    oa, ob, oc = _coeffs(o1, o2)
    u1 = _root(sa, sb, sc)
    u2 = _root(sa + oa, sb + ob, sc + oc)
    upd = np.where((o1 < u1) & (u2 > o1), u2, u1)
    upd = np.where(hy | hx, upd, inf)
    free = trav & ~seeds
    upd = np.where(free, upd, u)
    res = np.zeros_like(u)
    reached = free & np.isfinite(u)
    with np.errstate(invalid="ignore"):
        res[reached] = np.abs(u[reached] - upd[reached])
    return res, upd


class GoalSelector:
    """State that ``update_global_goal`` carries across calls (``dd_wt``, ``last_global_goal``, ``global_goals``)."""

    def __init__(self, args, full_hw, col_rad=None):
        self.args = args
        self.full_w, self.full_h = full_hw
        self.selem = disk(int(args.col_rad if col_rad is None else col_rad))
        self.reset()

    def reset(self):
        self.dd_wt = None
        self.value = None
        self.last_global_goal = None
        self.global_goals = None
        self.dd = None

    def update(self, full_obstacle, lmb, loc_rc, target_pred, collision_map, visited_vis):
        """full_obstacle = full_map[0] [W,H]; lmb = (gx1, gx2, gy1, gy2); loc_rc = agent cell in the local map;
        target_pred [w,h].  Returns the new ``global_goals``."""
        args = self.args
        trav = traversible_map(full_obstacle, self.selem, collision_map, visited_vis)
        r = int(np.clip(loc_rc[0] + lmb[0], 0, self.full_w - 1))
        c = int(np.clip(loc_rc[1] + lmb[2], 0, self.full_h - 1))
        dd_raw = geodesic_field(trav, (r, c))
        self.dd = fill_field(dd_raw)
        goal, value, self.wt_sum, self.kept_last, self.dd_wt = select_from_field(
            dd_raw, lmb, target_pred, args.dist_weight_temperature, args.map_resolution, self.dd_wt)
        self.value = value
        new_global_goal = [goal]
        if new_global_goal != self.last_global_goal:
            self.last_global_goal = self.global_goals
            self.global_goals = new_global_goal
        return self.global_goals


def fmm_set_goal(traversible, goal_rc):
    """FMMPlanner.set_goal (fmm_planner.py:55-67, scale 1, no auto_improve)."""
    traversible_ma = ma.masked_values(traversible * 1, 0)
    traversible_ma[int(goal_rc[0]), int(goal_rc[1])] = 0
    dd = fmm_ref.distance(traversible_ma, dx=1)
    return ma.filled(dd, np.max(dd) + 1)


def fmm_set_multi_goal(traversible, goal_map):
    """FMMPlanner.set_multi_goal (fmm_planner.py:69-75)."""
    traversible_ma = ma.masked_values(traversible * 1, 0)
    traversible_ma[goal_map == 1] = 0
    dd = fmm_ref.distance(traversible_ma, dx=1)
    return ma.filled(dd, np.max(dd) + 1)
