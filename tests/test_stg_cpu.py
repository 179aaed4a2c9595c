"""The short-term goal without a GPU: the host-side masks of ``peanut_stg_masks`` against the reference's ``get_mask`` / ``get_dist``,
and tests/stg_cases.py's NumPy restatement of ``_get_stg`` against what the reference's own code gave (tests/golden/stg_golden.npz,
written by tools/gen_golden_stg.py).  The scenes' claims are asserted so that the fixture cannot go hollow."""
import numpy as np
import pytest
from numpy import ma

import stg_cases as sc


@pytest.fixture(scope="module")
def golden():
    return np.load(sc.GOLDEN)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def test_abi_version_is_at_least_19():
    from peanut_amd import _lib
    assert _lib.ABI_VERSION >= 19
    assert _lib.load().peanut_abi_version() == _lib.ABI_VERSION


def test_host_masks_equal_the_references_bit_for_bit(golden):
    from peanut_amd.planner import stg_masks
    sweep = golden["b/sweep"]
    assert len(sweep) >= 100 and (sweep == 0.0).any() and (sweep == 0.5).any() and (sweep > 0.99).any()
    for k, (sx, sy) in enumerate(sweep):
        mask, dist = stg_masks(sx, sy, sc.STEP_SIZE)
        assert same_bits(mask, golden["b/get_mask"][k]), (sx, sy)
        assert same_bits(dist, golden["b/get_dist"][k]), (sx, sy)
    # the product's NumPy mirrors (peanut_amd.goal.get_mask / get_dist) are the same functions
    from peanut_amd import goal
    for k in (0, 17, 60, len(sweep) - 1):
        sx, sy = sweep[k]
        assert same_bits(goal.get_mask(sx, sy, 1.0, 5), golden["b/get_mask"][k]) and same_bits(goal.get_dist(sx, sy, 1.0, 5), golden["b/get_dist"][k])


def test_host_masks_refuse_bad_arguments():
    import ctypes as C
    from peanut_amd import _lib
    lib = _lib.load()
    buf = (C.c_double * 121)()
    assert lib.peanut_stg_masks(0.0, 0.0, 6, buf, buf) == -2 and lib.peanut_stg_masks(0.0, 0.0, 0, buf, buf) == -2
    assert lib.peanut_stg_masks(0.0, 0.0, 5, None, buf) == -2


def test_restatement_reproduces_every_mask_of_the_chain(golden):
    seen_retry, seen_magnify = set(), set()
    for c in sc.mask_cases():
        replies, _, _, want_retry, want_magnify = sc.SCRIPTS[c["script"]]
        got = sc.get_stg(c, sc.Script(replies))
        n, retried, n_magnify = golden[f"a/{c['name']}/n"]
        assert (got["n_solves"], got["retried"], got["n_magnify"]) == (n, retried, n_magnify) == (n, want_retry, want_magnify), c["name"]
        for k, (trav, goal) in enumerate(got["masks"]):
            assert np.array_equal(trav, golden[f"a/{c['name']}/trav{k}"]), f"{c['name']}: traversible map of solve {k}"
            assert np.array_equal(goal, golden[f"a/{c['name']}/goal{k}"]), f"{c['name']}: goal mask of solve {k}"
        for key in ("obstacle", "goal", "collision", "visited"):      # the fixture was generated from these very inputs
            assert np.array_equal(c[key], golden[f"a/{c['name']}/{key}"]), (c["name"], key)
        seen_retry.add(int(retried))
        seen_magnify.add(int(n_magnify))
    assert seen_retry == {0, 1} and seen_magnify >= {0, 1, 2, 8}


def test_mask_cases_cover_what_they_claim():
    cases = sc.mask_cases()
    assert {c["m"] for c in cases} == {61, 62, 45} and {c["col_rad"] for c in cases} == {0, 1, 3, 4}
    for key, want in ((0, {0, 1}), (1, {0, 1})):
        ints = {int(c["start_exact"][key]) for c in cases} | {int(c["start_exact"][key]) - c["m"] for c in cases}
        assert want | {-1} <= ints
    edges = set()
    for c in cases:
        gx1, gx2, gy1, gy2 = c["lmb"]
        edges |= {("gx1", gx1 == 0), ("gx2", gx2 == c["full"]), ("gy1", gy1 == 0), ("gy2", gy2 == c["full"])}
        assert gx2 - gx1 == c["m"] and gy2 - gy1 == c["m"]
    assert len(edges) == 8
    vals = np.concatenate([c["obstacle"][c["obstacle"] != 0] for c in cases])
    assert {0.5, 1.5} <= set(np.unique(vals).tolist()) and np.float32(0.500001) in vals
    both = sum(int(((c["collision"] == 1) & (c["visited"] == 1))[c["lmb"][0]:c["lmb"][1], c["lmb"][2]:c["lmb"][3]].sum()) for c in cases)
    assert both > 0
    # the two quirks each change at least one cell somewhere: the empty [-1:2] slice, and `grid[y1] = 1` being a row
    empty_slice = row_rule = 0
    for c in cases:
        grid = sc.bordered_grid(c["obstacle"], c["lmb"], c["full"], c["full"])
        trav = sc.traversible(grid, c["lmb"], c["col_rad"], c["collision"], c["visited"], c["start_exact"])[1:-1, 1:-1]
        i, j = int(c["start_exact"][0]), int(c["start_exact"][1])
        clipped = trav.copy()
        clipped[max(i - 1, 0):i + 2, max(j - 1, 0):j + 2] = 1
        empty_slice += int((clipped != trav).sum())
        if c["lmb"][2] == 0 and c["lmb"][0] != 0:
            col = np.rint(c["obstacle"]) != 0
            if c["lmb"][1] == c["full"]:
                col[-1] = True
            if c["lmb"][3] == c["full"]:
                col[:, -1] = True
            col[:, 0] = True                       # what `grid[:, y1] = 1` would have done
            row_rule += int((col != grid).sum())
    assert empty_slice > 0 and row_rule > 0


def oracle_plan(trav, goal, state):
    """FMMPlanner(trav).set_multi_goal(goal) + get_short_term_goal(state) with the oracle's field (oracle/fmm_ref.c) and the
    product's NumPy window."""
    from oracle import fmm_ref
    from peanut_amd.goal import FMMPlanner
    t = ma.masked_values(trav.astype(np.float64), 0)
    t[goal == 1] = 0
    dd = fmm_ref.distance(t, dx=1)
    dd = ma.filled(dd, np.max(dd) + 1)
    p = FMMPlanner.__new__(FMMPlanner)
    p.scale, p.step_size, p.du, p._host, p.fmm_dist_dev = 1, sc.STEP_SIZE, sc.STEP_SIZE, np.array(dd), None
    return p.get_short_term_goal(state)


def test_restatement_reproduces_the_scenes(golden):
    claims = {}
    for c in sc.scene_cases():
        got = sc.get_stg(c, oracle_plan)
        want = golden[f"c/{c['name']}/result"]
        assert got["stg"] == (want[0], want[1]) and got["stop"] == bool(want[2]), c["name"]
        assert (got["retried"], got["n_magnify"], got["n_solves"]) == (want[3], want[4], want[5]), c["name"]
        assert same_bits(got["distance"], want[6]) and got["replan"] == bool(want[7]), c["name"]
        assert got["retried"] == c["expect_retry"], c["name"]
        if c["expect_magnify"] is not None:
            assert got["n_magnify"] == c["expect_magnify"], c["name"]
        claims[c["name"]] = (got["retried"], got["n_magnify"])
    assert claims == {"doors": (0, 0), "behind_wall": (0, 0), "unreachable": (1, 0), "blocked_start": (1, 0), "serpentine_toilet": (0, 2),
                      "serpentine_chair": (0, 8), "serpentine_shortcut": (0, 2)}


def test_window_fixture_covers_what_it_claims(golden):
    r = golden["b/results"]
    cases = sc.window_cases()
    assert len(r) == len(cases) and all(r[k, 0] == s[0] and r[k, 1] == s[1] for k, (_, _, s) in enumerate(cases))
    stop, replan = r[:, 5] == 1, r[:, 6] == 1
    assert stop.any() and (~stop).any() and replan.any() and (~replan).any()
    names = [c[0] for c in cases]
    by = {n: r[k] for k, n in enumerate(names)}
    # 4.999... stops, 5.0 does not
    assert all(by[f"near5_30_{k}"][5] == 1 and by[f"near5_40_{k}"][5] == 0 for k in range(4))
    assert by["near5_30_0"][4] == np.nextafter(5.0, 0.0) and by["near5_40_0"][4] == 5.0
    # a minimum of exactly -0.0001 and its two neighbours fall on both sides of `> -0.0001`
    for name in ("threshold", "threshold8"):
        sides = {(b, bool(by[f"{name}_10_{b}"][6])) for b in (5, 26, 47)}
        assert {s for _, s in sides} == {True, False}, sides
    # NaN: a NaN on the ring wins, a NaN centre gives a NaN distance
    assert np.isnan(by["nan_45_45"][4]) and (by["nan_30_30"][2], by["nan_30_30"][3]) == (31.0, 33.0)
    # the pad value entered: a chosen cell never lies outside the field
    assert (r[:, 2] >= 0).all() and (r[:, 3] >= 0).all()
