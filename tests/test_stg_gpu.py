"""The short-term goal on the device (csrc/stg.hip, peanut_amd/planner.py) against tests/golden/stg_golden.npz: what the reference's
OWN ``Agent_Helper._get_stg`` and ``FMMPlanner.get_short_term_goal`` gave on the cases of tests/stg_cases.py
(tools/gen_golden_stg.py).  Masks, windows and the composite around the device field are compared bit for bit; the scenes, whose
expectations come from the oracle's field (oracle/fmm_ref.c, up to the 0.5-cell gate of tests/test_goal_gpu.py from the device's),
were admitted with a whole cell of margin on every decision and are compared in ``stg``, ``stop``, ``retried`` and ``n_magnify``."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stg_cases as sc                 # noqa: E402
import workspace_cases as wc           # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from peanut_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    return np.load(sc.GOLDEN)


def _upload(c):
    """A case with its maps on the device (never written); the obstacle also as a strided view into a larger tensor."""
    c = dict(c)
    m = c["m"]
    c["obstacle_dev"] = torch.from_numpy(c["obstacle"]).cuda()
    big = torch.full((m + 3, m + 5), 9.0, dtype=torch.float32, device="cuda")
    big[2:m + 2, 4:m + 4] = c["obstacle_dev"]
    c["obstacle_view"] = big[2:m + 2, 4:m + 4]
    for k in ("goal", "collision", "visited"):
        c[k + "_dev"] = torch.from_numpy(c[k]).cuda()
    return c


@pytest.fixture(scope="module")
def mask_cases():
    return [_upload(c) for c in sc.mask_cases()]


@pytest.fixture(scope="module")
def scenes():
    return [_upload(c) for c in sc.scene_cases()]


_PLANNERS = {}


def planner_for(c, fresh=False):
    from peanut_amd.planner import ShortTermGoal
    key = (c["m"], c["col_rad"])
    if fresh or key not in _PLANNERS:
        args = SimpleNamespace(map_size_cm=c["full"] * 5, map_resolution=5, global_downscaling=2, col_rad=c["col_rad"],
                               magnify_goal_when_hard=c.get("magnify_when_hard", sc.MAGNIFY_WHEN_HARD))
        p = ShortTermGoal(args, device="cuda:0")
        if fresh:
            return p
        _PLANNERS[key] = p
    return _PLANNERS[key]


def run(p, c, taps=True, obstacle=None):
    p.get_stg(c["obstacle_dev"] if obstacle is None else obstacle, c["goal_dev"], c["collision_dev"], c["visited_dev"], c["lmb"],
              c["start_exact"], c["found_goal"], c["goal_name"], taps=taps)
    return p.last


# ---- (a) the masks ----
def test_traversible_map_equals_the_reference_with_and_without_the_erosion(mask_cases, golden):
    from peanut_amd.planner import stg_traversible
    eroded = 0
    for c in mask_cases:
        n_solves, retried, _ = golden[f"a/{c['name']}/n"]
        for obst in (c["obstacle_dev"], c["obstacle_view"]):
            assert obst is c["obstacle_dev"] or not obst.is_contiguous()
            got = stg_traversible(obst, (c["full"], c["full"]), c["lmb"], c["col_rad"], c["collision_dev"], c["visited_dev"], c["start_exact"])
            assert np.array_equal(got.cpu().numpy(), golden[f"a/{c['name']}/trav0"]), c["name"]
            if retried:
                got = stg_traversible(obst, (c["full"], c["full"]), c["lmb"], c["col_rad"], c["collision_dev"], c["visited_dev"],
                                      c["start_exact"], erode=True)
                assert np.array_equal(got.cpu().numpy(), golden[f"a/{c['name']}/trav1"]), c["name"]
                eroded += 1
        assert torch.equal(c["obstacle_view"], c["obstacle_dev"])        # read in place, never written
    assert eroded >= 6


def test_goal_mask_equals_the_reference_from_padded_and_unpadded_input(mask_cases, golden):
    from peanut_amd.planner import stg_goal
    steps = 0
    for c in mask_cases:
        n_solves, retried, n_magnify = golden[f"a/{c['name']}/n"]
        radius = sc.toilet_rule(c["goal_name"])[0] if c["found_goal"] == 1 else 2
        want = golden[f"a/{c['name']}/goal0"]
        got = stg_goal(c["goal_dev"], radius)
        assert np.array_equal(got.cpu().numpy(), want), c["name"]
        padded = torch.from_numpy(sc.add_boundary(c["goal"], 0)).cuda()
        assert np.array_equal(stg_goal(padded, radius, padded=True).cpu().numpy(), want), c["name"]
        for k in range(int(n_solves - n_magnify), int(n_solves)):           # the magnify loop: disk(2) on the padded mask
            got = stg_goal(got, 2, padded=True)
            assert np.array_equal(got.cpu().numpy(), golden[f"a/{c['name']}/goal{k}"]), (c["name"], k)
            steps += 1
    assert steps >= 20


# ---- (b) the window ----
def _windows(lib, field, states, step=sc.STEP_SIZE):
    """peanut_stg_window for every state on one device field -> list of (stg_r, stg_c, distance, stop, replan); one read-back."""
    from peanut_amd import _lib
    size = C.sizeof(_lib.StgWindowC)
    res = torch.full((len(states) * size,), 0xA5, dtype=torch.uint8, device="cuda")
    for k, s in enumerate(states):
        rc = lib.peanut_stg_window(field.data_ptr(), int(field.shape[0]), float(s[0]), float(s[1]), step, res.data_ptr() + k * size,
                                   _lib.current_stream_ptr())
        _lib.check(rc, "peanut_stg_window")
    raw = res.cpu().numpy().tobytes()
    out = [_lib.StgWindowC.from_buffer_copy(raw[k * size:(k + 1) * size]) for k in range(len(states))]
    return [(w.stg_r, w.stg_c, w.distance, w.stop, w.replan) for w in out]


def test_window_equals_the_reference_in_all_five_outputs(lib, golden):
    cases = sc.window_cases()
    want = golden["b/results"]
    fields = {k: torch.from_numpy(golden[f"b/field/{k}"]).cuda() for k in sc.window_fields()}
    for key, field in fields.items():
        idx = [k for k, c in enumerate(cases) if c[1] == key]
        got = _windows(lib, field, [cases[k][2] for k in idx])
        for k, g in zip(idx, got):
            w = want[k]
            assert (float(g[0]), float(g[1]), g[3], g[4]) == (w[2], w[3], int(w[5]), int(w[6])), (cases[k][0], g, w)
            assert np.float64(g[2]).tobytes() == np.float64(w[4]).tobytes(), (cases[k][0], g[2], w[4])


def test_planner_window_on_the_device_equals_its_numpy_form(scenes):
    from peanut_amd.goal import FMMPlanner
    c = scenes[0]
    grid = sc.bordered_grid(c["obstacle"], c["lmb"], c["full"], c["full"])
    trav = sc.traversible(grid, c["lmb"], c["col_rad"], c["collision"], c["visited"], c["start_exact"])
    goal = sc.dilate_goal(sc.add_boundary(c["goal"], 0), 2)
    p = FMMPlanner(torch.from_numpy(trav).cuda())
    p.set_multi_goal(torch.from_numpy(goal).cuda())
    for state in ([15.5, 9.5], [1.0, 1.25], [62.999, 62.0], [51.5, 20.75], [11.0, 31.999999]):
        a, b = p.get_short_term_goal_dev(state), p.get_short_term_goal(state)
        assert wc.same([float(a[0]), float(a[1]), float(a[2]), a[3], a[4]], [float(b[0]), float(b[1]), float(b[2]), b[3], b[4]]), (state, a, b)


# ---- the composite ----
def _device_plan(solver_cache):
    """plan(trav, goal, state) of stg_cases.get_stg: peanut_fmm_distance (fill 1) on the two masks, then the NumPy window."""
    from peanut_amd.goal import FMMPlanner, GeodesicSolver
    fields = []

    def plan(trav, goal, state):
        n = trav.shape[0]
        if n not in solver_cache:
            solver_cache[n] = GeodesicSolver(n, n, 0)
        p = FMMPlanner(torch.from_numpy(np.ascontiguousarray(trav)).cuda(), solver=solver_cache[n], step_size=sc.STEP_SIZE)
        p.set_multi_goal(torch.from_numpy(np.ascontiguousarray(goal)).cuda())
        fields.append(p.fmm_dist_dev)
        return p.get_short_term_goal(state)
    return plan, fields


def _result(last):
    return {k: last[k] for k in ("stg", "distance", "stop", "replan", "retried", "n_magnify", "n_solves")}


def test_plan_equals_the_composition_of_its_parts_bit_for_bit(mask_cases, scenes, golden):
    solvers = {}
    flows = set()
    for c in mask_cases + scenes:
        plan, fields = _device_plan(solvers)
        want = sc.get_stg(c, plan)
        got = run(planner_for(c), c)
        masks = want.pop("masks")
        assert wc.same(_result(got), want), (c["name"], _result(got), want)
        assert wc.same(got["dist"], fields[-1]), wc.first_difference(got["dist"], fields[-1], c["name"])
        assert np.array_equal(got["trav"].cpu().numpy(), masks[-1][0]) and np.array_equal(got["goal"].cpu().numpy(), masks[-1][1]), c["name"]
        if f"a/{c['name']}/n" in golden:                    # the chain's masks are the reference's wherever the chains coincide
            n, retried, n_magnify = golden[f"a/{c['name']}/n"]
            assert np.array_equal(masks[0][0], golden[f"a/{c['name']}/trav0"]) and np.array_equal(masks[0][1], golden[f"a/{c['name']}/goal0"])
            if (want["retried"], want["n_magnify"]) == (retried, n_magnify):
                assert np.array_equal(got["trav"].cpu().numpy(), golden[f"a/{c['name']}/trav{n - 1}"])
                assert np.array_equal(got["goal"].cpu().numpy(), golden[f"a/{c['name']}/goal{n - 1}"])
        flows.add((want["retried"], min(want["n_magnify"], 1)))
    assert flows >= {(0, 0), (1, 0), (0, 1)}, flows      # plain, retried and magnified chains were all compared


def test_every_scene_ends_where_the_reference_ends(scenes, golden):
    for c in scenes:
        got = run(planner_for(c), c)
        want = golden[f"c/{c['name']}/result"]
        print(f"{c['name']}: stg {got['stg']} stop {got['stop']} retried {got['retried']} magnify {got['n_magnify']} "
              f"distance {got['distance']!r} (oracle field: {want[6]!r})")
        assert got["stg"] == (want[0], want[1]) and got["stop"] == bool(want[2]), c["name"]
        assert (got["retried"], got["n_magnify"]) == (want[3], want[4]), c["name"]
        assert abs(got["distance"] - want[6]) <= 0.5, c["name"]      # the project's field gate


# ---- the agent ----
def _agent_args(**over):
    from oracle.agent_ref import agent_args
    base = dict(only_explore=0, map_size_cm=1200, vision_range=48, prediction_window=240, num_local_steps=3, update_goal_freq=4,
                select_goal=True, goal_map=True, goal_erode=3, plan_stg=True)
    base.update(over)
    return agent_args(**base)


class _FakePrediction:
    def __init__(self, size):
        from oracle.agent_ref import fake_pattern
        self.pattern = torch.from_numpy(fake_pattern(size=size)).cuda()

    def get_prediction_batch(self, maps, apply_sigmoid=True, out=None):
        return torch.tanh(maps[:, [0, 1, 4, 5, 6, 7]] + self.pattern[None]) * 0.5 + 0.5


def test_agent_state_and_act_give_the_stand_alone_result_and_nothing_with_the_switch_off():
    from oracle import mapping_scenes
    from peanut_amd.peanut_agent import PEANUT_Agent
    from peanut_amd.planner import ShortTermGoal
    for on in (True, False):
        args = _agent_args(plan_stg=on)
        agent = PEANUT_Agent(args, prediction_model=_FakePrediction(args.prediction_window))
        agent.reset()
        alone = ShortTermGoal(args, device="cuda:0") if on else None
        for i, fr in enumerate(mapping_scenes.make_sequence(seed=3, n_frames=4)):
            out = agent.act({"gps": np.array([0.1 * i, 0.0], np.float32), "compass": np.array([0.0], np.float32),
                             "objectgoal": np.array([4]), "obs": torch.from_numpy(mapping_scenes.frame_to_obs(fr))[None]})
            assert ("stg" in out) == on and ("stop" in out) == on
            st = agent.agent_states
            if not on:
                assert st.stg is None and st._stg is None
                with pytest.raises(RuntimeError):
                    st.short_term_goal({"goal_name": out["goal_name"]})
                continue
            pose = st.planner_pose_inputs
            lmb = [int(v) for v in pose[3:]]
            start = [pose[1] * 100.0 / args.map_resolution - lmb[0], pose[0] * 100.0 / args.map_resolution - lmb[2]]
            want = alone.get_stg(st.local_map[0], st.goal_map, st.collision_map, st.visited_vis, lmb, start, st.found_goal, out["goal_name"])
            assert wc.same((out["stg"], out["stop"]), want) and wc.same(st._stg.last, alone.last), (i, st._stg.last, alone.last)
            assert wc.same(st.short_term_goal({"goal_name": out["goal_name"]}), want)
    with pytest.raises(ValueError):
        args = _agent_args(goal_map=False)
        agent = PEANUT_Agent(args, prediction_model=_FakePrediction(args.prediction_window))
        agent.reset()
        fr = mapping_scenes.make_sequence(seed=3, n_frames=1)[0]
        agent.act({"gps": np.zeros(2, np.float32), "compass": np.zeros(1, np.float32), "objectgoal": np.array([4]),
                   "obs": torch.from_numpy(mapping_scenes.frame_to_obs(fr))[None]})


# ---- no result depends on what the workspace held ----
def test_results_do_not_depend_on_the_handles_history(scenes):
    by = {c["name"]: c for c in scenes}
    a, b = by["serpentine_shortcut"], by["serpentine_chair"]      # the same handle size, other chains
    fresh = planner_for(a, fresh=True)
    want = dict(run(fresh, a))
    with wc.poisoned():
        poisoned = planner_for(a, fresh=True)
        got = dict(run(poisoned, a))
    assert wc.same(got, want), wc.first_difference(got, want)
    used = planner_for(a, fresh=True)
    run(used, b)
    got = dict(run(used, a))
    assert wc.same(got, want), wc.first_difference(got, want)
    refused = planner_for(a, fresh=True)
    from peanut_amd import _lib
    with pytest.raises(_lib.PeanutHipError):
        refused.get_stg(a["obstacle_dev"], a["goal_dev"], a["collision_dev"], a["visited_dev"], a["lmb"], [-0.5, 3.0], 1, "chair")
    got = dict(run(refused, a))
    assert wc.same(got, want), wc.first_difference(got, want)


# ---- refusals ----
def test_plan_refuses_bad_arguments_before_anything_is_enqueued(lib, scenes):
    from peanut_amd import _lib
    c = scenes[0]
    m, full, n = c["m"], c["full"], c["m"] + 2
    p = planner_for(c, fresh=True)
    taps = [torch.full((n, n), 0x5A, dtype=torch.uint8, device="cuda"), torch.full((n, n), 0x5A, dtype=torch.uint8, device="cuda"),
            torch.full((n, n), -7.0, dtype=torch.float64, device="cuda")]
    keep = [t.clone() for t in taps]
    small = C.c_void_p()
    _lib.check(lib.peanut_stg_create(C.byref(small), 9, 18, 18, 1, 5), "peanut_stg_create")      # m < 2 step_size + 1
    wide = C.c_void_p()
    _lib.check(lib.peanut_stg_create(C.byref(wide), m, full, full, 17, 5), "peanut_stg_create")  # col_rad above the limit

    def call(h=None, obstacle=c["obstacle_dev"].data_ptr(), stride=m, goal=c["goal_dev"].data_ptr(), col=c["collision_dev"].data_ptr(),
             vis=c["visited_dev"].data_ptr(), lmb=c["lmb"], start=c["start_exact"], radius=8, result=True, start_null=False, lmb_null=False):
        res = _lib.StgResultC()
        C.memset(C.byref(res), 0x6B, C.sizeof(res))
        before = bytes(res)
        rc = lib.peanut_stg_plan(p._h if h is None else h, obstacle, stride, goal, col, vis, None if lmb_null else C.byref((C.c_int * 4)(*lmb)),
                                 None if start_null else C.byref((C.c_double * 2)(*start)), 1, radius, 100.0, 8, C.byref(res) if result else None,
                                 taps[0].data_ptr(), taps[1].data_ptr(), taps[2].data_ptr(), _lib.current_stream_ptr())
        torch.cuda.synchronize()
        assert bytes(res) == before and all(torch.equal(t, k) for t, k in zip(taps, keep))
        return rc

    gx1, gx2, gy1, gy2 = c["lmb"]
    bad = dict(null_handle=dict(h=C.c_void_p()), null_obstacle=dict(obstacle=None), null_goal=dict(goal=None), null_collision=dict(col=None),
               null_visited=dict(vis=None), null_lmb=dict(lmb_null=True), null_start=dict(start_null=True), null_result=dict(result=False),
               small_m=dict(h=small, lmb=[0, 9, 0, 9], start=[4.0, 4.0], stride=9), lmb_size=dict(lmb=[gx1, gx2 - 1, gy1, gy2]),
               lmb_outside=dict(lmb=[gx1 + full, gx2 + full, gy1, gy2]), lmb_negative=dict(lmb=[-1, m - 1, gy1, gy2]),
               start_negative=dict(start=[-0.25, 5.0]), start_beyond=dict(start=[5.0, float(m)]), start_nan=dict(start=[float("nan"), 5.0]),
               radius=dict(radius=17), col_rad=dict(h=wide), stride=dict(stride=m - 1))
    for name, kw in bad.items():
        assert call(**kw) == -2, name
    run(p, c)                       # the handle that refused all of these still plans
    lib.peanut_stg_destroy(small)
    lib.peanut_stg_destroy(wide)


def test_operators_refuse_bad_arguments(lib, mask_cases):
    from peanut_amd import _lib
    c = mask_cases[0]
    m = c["m"]
    out = torch.full((m + 2, m + 2), 0x5A, dtype=torch.uint8, device="cuda")
    keep = out.clone()
    s = _lib.current_stream_ptr()
    lmb = C.byref((C.c_int * 4)(*c["lmb"]))
    o, col, vis = c["obstacle_dev"].data_ptr(), c["collision_dev"].data_ptr(), c["visited_dev"].data_ptr()
    assert lib.peanut_stg_traversible(o, m, m, c["full"], c["full"], lmb, 17, 0, col, vis, 3, 3, out.data_ptr(), s) == -2
    assert lib.peanut_stg_traversible(o, m - 1, m, c["full"], c["full"], lmb, 4, 0, col, vis, 3, 3, out.data_ptr(), s) == -2
    assert lib.peanut_stg_traversible(o, m, m, c["full"], c["full"], lmb, 4, 0, col, vis, m, 3, out.data_ptr(), s) == -2
    assert lib.peanut_stg_traversible(o, m, m, c["full"], c["full"], lmb, 4, 0, col, vis, 3, -1, out.data_ptr(), s) == -2
    assert lib.peanut_stg_traversible(o, m, m, c["full"], c["full"], lmb, 4, 0, col, vis, 3, 3, None, s) == -2
    assert lib.peanut_stg_goal(c["goal_dev"].data_ptr(), 0, m, 17, out.data_ptr(), s) == -2
    assert lib.peanut_stg_goal(out.data_ptr(), 1, m, 2, out.data_ptr(), s) == -2
    field = torch.zeros((m + 2, m + 2), dtype=torch.float64, device="cuda")
    for state, step in (((-1.0, 3.0), 5), ((3.0, float(m + 2)), 5), ((3.0, 3.0), 6), ((3.0, 3.0), 0), ((float("nan"), 3.0), 5)):
        assert lib.peanut_stg_window(field.data_ptr(), m + 2, state[0], state[1], step, out.data_ptr(), s) == -2
    torch.cuda.synchronize()
    assert torch.equal(out, keep)
