"""The batched short-term goal without a GPU: the binding (ABI 20, the descriptor's layout), the grouping of lock-step episodes, and
the two scenes tests/stg_batch_cases.py adds -- run through stg_cases' restatement of ``_get_stg`` on the oracle's field, the way
tests/test_stg_cpu.py runs the scenes of stg_cases, with the whole-cell margin of tools/gen_golden_stg.py (check_margins) asserted on
every decision of every solve, so that the device's field (within 0.5 cell of the oracle's) takes the same chain."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import stg_batch_cases as bc
import stg_cases as sc
from test_stg_cpu import oracle_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_version_is_at_least_20_and_the_batch_symbols_are_bound():
    from peanut_amd import _lib
    assert _lib.ABI_VERSION >= 20
    lib = _lib.load()
    assert lib.peanut_abi_version() == _lib.ABI_VERSION
    assert lib.peanut_stg_plan_batch.argtypes == [C.POINTER(_lib.StgBatchC)] and lib.peanut_stg_waves.restype == C.c_int
    # refusals that need no device: a null descriptor, a wrong size, E out of range, null arrays
    assert lib.peanut_stg_plan_batch(None) == -2
    for d in (_lib.StgBatchC(size=C.sizeof(_lib.StgBatchC) - 8, E=1), _lib.StgBatchC(size=C.sizeof(_lib.StgBatchC), E=0),
              _lib.StgBatchC(size=C.sizeof(_lib.StgBatchC), E=17), _lib.StgBatchC(size=C.sizeof(_lib.StgBatchC), E=2)):
        assert lib.peanut_stg_plan_batch(C.byref(d)) == -2
    assert lib.peanut_stg_waves(None) == -2


def test_descriptor_layout_equals_the_headers():
    """sizeof and every offset of the ctypes struct, from the header's own field list under the C layout rules of the platform
    (every field here is a pointer, a 64-bit or a 32-bit integer)."""
    from peanut_amd import _lib
    with open(os.path.join(ROOT, "include", "peanut_hip.h"), encoding="utf-8") as f:
        src = f.read()
    body = re.search(r"typedef struct \{([^}]*)\} peanut_stg_batch_t;", src).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in [d.strip() for d in body.split(";") if d.strip()]:
        if "*" in decl:
            fields.append((decl.rsplit("*", 1)[1].strip(), C.sizeof(C.c_void_p)))
        else:
            typ, names = decl.split(None, 1)
            size = {"uint64_t": 8, "int32_t": 4}[typ]
            fields += [(n.strip(), size) for n in names.split(",")]
    offset, align, want = 0, 1, {}
    for name, size in fields:
        offset = (offset + size - 1) // size * size
        want[name] = offset
        offset += size
        align = max(align, size)
    total = (offset + align - 1) // align * align
    assert [n for n, _ in fields] == [n for n, _ in _lib.StgBatchC._fields_]
    assert fields[0][0] == "size" and fields[-1][0] == "stream"
    assert {n: getattr(_lib.StgBatchC, n).offset for n, _ in fields} == want
    assert C.sizeof(_lib.StgBatchC) == total == 152
    assert re.search(r"#define PEANUT_STG_MAX_BATCH PEANUT_GOAL_MAX_BATCH", src) and re.search(r"#define PEANUT_GOAL_MAX_BATCH 16\b", src)
    from peanut_amd import planner
    assert planner.MAX_BATCH == 16


def _state(local=240, full=480, col_rad=4, plan=True, step=None):
    s = SimpleNamespace(local_w=local, local_h=local, full_w=full, full_h=full, args=SimpleNamespace(col_rad=col_rad, plan_stg=plan))
    if step is not None:
        s._stg = SimpleNamespace(step_size=step)
    return s


def test_stg_batch_groups_on_map_sizes_col_rad_and_step_size():
    from peanut_amd.agent_state import Agent_State_Group as G
    a, b, c = _state(), _state(), _state()
    assert G._stg_batch([]) == []
    assert G._stg_batch([a]) == [[a]]
    assert G._stg_batch([a, b, c]) == [[a, b, c]]
    d, e, f, g = _state(local=120), _state(full=960), _state(col_rad=3), _state(step=4)
    got = G._stg_batch([a, d, b, e, f, c, g])
    assert got == [[a, b, c], [d], [e], [f], [g]]                  # in the order of the first members; members keep their order
    assert G._stg_batch([a, _state(step=5), _state(step=None)])[0][0] is a and len(G._stg_batch([a, _state(step=5)])) == 1
    many = [_state() for _ in range(35)]
    got = G._stg_batch(many)
    assert [len(x) for x in got] == [16, 16, 3] and [s for x in got for s in x] == many
    assert G.STG_BATCH_MIN >= 2


def margins(field, state, magnify_when_hard):
    """tools/gen_golden_stg.py's check_margins on the product's NumPy masks: every decision taken on this solve keeps more than a
    whole cell (0.2 for the ratio) from its threshold; a window that lies on the plateau of unreached cells is exempt where the
    plateau itself decides (all its cells are equal on any field)."""
    from peanut_amd import goal
    n, du = field.shape[0], sc.STEP_SIZE
    ir, ic = int(state[0]), int(state[1])
    mask, dist_mask = goal.get_mask(state[0] - ir, state[1] - ic, 1.0, du), goal.get_dist(state[0] - ir, state[1] - ic, 1.0, du)
    raw = np.pad(field, du, 'constant', constant_values=n ** 2)[ir:ir + 2 * du + 1, ic:ic + 2 * du + 1].copy()
    top = field.max()
    unreached = (np.pad(field, du, 'constant', constant_values=-1)[ir:ir + 2 * du + 1, ic:ic + 2 * du + 1] == top) & (np.sum(field == top) > 1)
    centre = raw[du, du]
    sub = raw * mask + (1 - mask) * n ** 2 - centre
    ratio = sub / dist_mask
    assert np.all(np.abs(ratio[mask == 1] + 1.5) > 0.2), "a ratio within 0.2 of -1.5"
    sub[ratio < -1.5] = 1
    order = np.argsort(sub, axis=None, kind="stable")
    best, second = np.unravel_index(order[0], sub.shape), np.unravel_index(order[1], sub.shape)
    plateau_tie = unreached[best] and unreached[second] and unreached[du, du]
    assert plateau_tie or sub[second] - sub[best] > 1.0, f"the best cell leads by {sub[second] - sub[best]}"
    assert (unreached[best] and unreached[du, du] and sub[best] == 0) or abs(sub[best] + 0.0001) > 1.0, f"minimum {sub[best]}"
    assert abs(centre - 5.0) > 1.0, f"centre {centre}"
    assert abs(centre - 100) > 1.0 and abs(centre - magnify_when_hard) > 1.0, f"distance {centre}"


def oracle_field(trav, goal):
    from numpy import ma
    from oracle import fmm_ref
    t = ma.masked_values(trav.astype(np.float64), 0)
    t[goal == 1] = 0
    dd = fmm_ref.distance(t, dx=1)
    return np.array(ma.filled(dd, np.max(dd) + 1))


@pytest.fixture(scope="module")
def new_chains():
    """The two new scenes on the oracle's field, margins asserted on every solve -> {name: result of stg_cases.get_stg}."""
    out = {}
    for c in bc.new_scenes():
        def plan(trav, goal, state, c=c):
            margins(oracle_field(trav, goal), state, sc.MAGNIFY_WHEN_HARD)
            return oracle_plan(trav, goal, state)
        out[c["name"]] = sc.get_stg(c, plan)
    return out


def test_new_scenes_take_their_chains_with_a_whole_cell_of_margin(new_chains):
    by = {c["name"]: c for c in bc.new_scenes()}
    assert set(by) == {"plugged_corridor", "plugged_serpentine"}
    for name, got in new_chains.items():
        c = by[name]
        assert c["m"] == 62 and c["col_rad"] == 0
        assert got["retried"] == c["expect_retry"] == 1 and got["n_magnify"] == c["expect_magnify"], (name, got["retried"], got["n_magnify"])
        # the walls are the collision map and the plug is ONE obstacle cell, which the erosion removes: the retry's map differs from
        # the first in the plug alone
        assert int((np.rint(c["obstacle"]) != 0).sum()) == 1
        first, retry = got["masks"][0][0], got["masks"][1][0]
        pr, pc = np.argwhere(np.rint(c["obstacle"]) != 0)[0]
        assert first[pr + 1, pc + 1] == 0 and retry[pr + 1, pc + 1] == 1 and int((first != retry).sum()) == 1
    assert (new_chains["plugged_corridor"]["n_solves"], new_chains["plugged_serpentine"]["n_solves"]) == (2, 10)
    assert new_chains["plugged_corridor"]["replan"] is False and new_chains["plugged_serpentine"]["distance"] > 101.0


def test_corridors_of_the_new_scenes_are_one_cell_wide():
    for c in bc.new_scenes():
        free = sc._local(c, "collision") != 1
        # no 2 x 2 block of free cells anywhere: the walk never widens
        assert not (free[:-1, :-1] & free[1:, :-1] & free[:-1, 1:] & free[1:, 1:]).any(), c["name"]


def test_the_full_group_holds_every_chain(new_chains):
    golden = np.load(sc.GOLDEN)
    group = bc.groups()[bc.FULL_GROUP]
    names = [c["name"] for c in group]
    assert names[:5] == ["serpentine_toilet", "serpentine_chair", "serpentine_shortcut", "plugged_corridor", "plugged_serpentine"]
    assert len(names) == 6 and names[5].startswith("a04")
    solves, retried, magnify = {}, {}, {}
    for c in group[:5]:
        if c["name"] in new_chains:
            r = new_chains[c["name"]]
            solves[c["name"]], retried[c["name"]], magnify[c["name"]] = r["n_solves"], r["retried"], r["n_magnify"]
        else:
            want = golden[f"c/{c['name']}/result"]
            solves[c["name"]], retried[c["name"]], magnify[c["name"]] = int(want[5]), int(want[3]), int(want[4])
    assert solves == {"serpentine_toilet": 3, "serpentine_chair": 9, "serpentine_shortcut": 3, "plugged_corridor": 2, "plugged_serpentine": 10}
    assert len(set(solves.values())) >= 4 and any(retried.values()) and 8 in magnify.values()
    assert max(solves.values()) == 10        # the longest chain _get_stg can take: first, retry, eight steps


def test_groups_have_the_sizes_the_gpu_tests_use():
    g = bc.groups()
    assert [len(g[k]) for k in (bc.FULL_GROUP, bc.PAIR_GROUP, bc.TRIPLE_GROUP, bc.RAGGED_GROUP)] == [6, 2, 3, 2]
    assert {c["name"] for c in g[bc.PAIR_GROUP]} >= {"blocked_start"} and {c["name"] for c in g[bc.TRIPLE_GROUP]} >= {"doors"}
    for key, cases in g.items():
        assert all(bc.group_key(c) == key for c in cases)
    v = bc.variants16()
    assert len(v) == 16 and len({c["name"] for c in v}) == 16 and all(bc.group_key(c) == bc.RAGGED_GROUP for c in v)
    assert len({(tuple(c["start_exact"]), c["goal"].tobytes()) for c in v}) == 16
    for c in v:
        assert 0 <= c["start_exact"][0] < c["m"] and 0 <= c["start_exact"][1] < c["m"] and c["goal"].any()
