"""peanut_goal_map / peanut_goal_map_batch (csrc/goal_map.hip) and what is built on them -- Agent_State.update_goal_map,
planner_inputs, the lock-step group's one batched call, PEANUT_Agent.act -- against tests/golden/goal_map_golden.npz: the
reference's OWN Agent_State.update_goal_map (agent_state.py:418-446, scikit-image's morphology as the scipy calls it makes).
Everything is compared bit for bit: the rule is binary morphology and one fp32 comparison evaluated in a stated order.

The agent-level tests compare with tests/goal_map_cases.goal_map_ref (held to the golden by tests/test_goal_map_cpu.py) on the
maps the episode actually produced."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import goal_map_cases as gmc      # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from peanut_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def cases():
    """Every case with its map on the device and the golden result; built once, never written."""
    golden = gmc.load_golden()
    out = []
    for c in gmc.all_cases():
        c = dict(c)
        c["dev"] = torch.from_numpy(c["local_map"]).cuda()
        c["want"], c["want_found"] = golden[c["name"]]
        out.append(c)
    return out


def _params(c):
    return [c["cn"], c["morph"], c["n_erode"], c["detect"], c["goal"][0], c["goal"][1]]


def _single(lib, lm, params, out=None, found=None, fill=None):
    """One peanut_goal_map call on ``lm`` [C, m, m] (any plane / row stride) -> (goal_map uint8 numpy, found)."""
    from peanut_amd import _lib
    m = int(lm.shape[1])
    if out is None:
        # the call must not depend on what its outputs held
        out = torch.full((m, m), 7 if fill is None else fill, dtype=torch.uint8, device="cuda")
        found = torch.full((1,), -5, dtype=torch.int32, device="cuda")
    rc = lib.peanut_goal_map(lm.data_ptr(), int(lm.shape[0]), m, int(lm.stride(0)), int(lm.stride(1)), *params, out.data_ptr(),
                             found.data_ptr(), _lib.current_stream_ptr())
    _lib.check(rc, "peanut_goal_map")
    return out.cpu().numpy(), int(found.cpu()[0])


def _batch(lib, maps, params, outs, found):
    from peanut_amd import _lib
    E = len(maps)
    ptrs = (C.c_void_p * E)(*[t.data_ptr() for t in maps])
    ps = (C.c_longlong * E)(*[int(t.stride(0)) for t in maps])
    rs = (C.c_longlong * E)(*[int(t.stride(1)) for t in maps])
    pr = (C.c_int * (6 * E))(*[int(v) for p in params for v in p])
    op = (C.c_void_p * E)(*[t.data_ptr() for t in outs])
    return lib.peanut_goal_map_batch(E, ptrs, int(maps[0].shape[0]), int(maps[0].shape[1]), ps, rs, pr, op, found.data_ptr(),
                                     _lib.current_stream_ptr())


def test_single_call_equals_the_reference_on_every_case(lib, cases):
    for c in cases:
        gm, found = _single(lib, c["dev"], _params(c))
        assert found == c["want_found"], c["name"]
        assert np.array_equal(gm, c["want"]), (c["name"], int(gm.sum()), int(c["want"].sum()))
        assert torch.equal(c["dev"].cpu(), torch.from_numpy(c["local_map"])), c["name"]        # the map is only read


@pytest.mark.parametrize("E", [1, 3, 16])
def test_batches_equal_the_single_calls(lib, cases, E):
    """The cases in batches of E (per map size), per-episode parameters differing; outputs pre-filled with other values.
    Contiguous maps only: every episode has the same strides here (the next test mixes them)."""
    for m in (gmc.M, gmc.M_RANDOM):
        group = [c for c in cases if c["local_map"].shape[1] == m]
        for lo in range(0, len(group), E):
            part = group[lo:lo + E]
            if len(part) < E:                                       # the last batch is filled up from the front, mixed order
                part = part + group[:E - len(part)][::-1]
            outs = [torch.full((m, m), 9, dtype=torch.uint8, device="cuda") for _ in part]
            found = torch.full((E,), -1, dtype=torch.int32, device="cuda")
            rc = _batch(lib, [c["dev"] for c in part], [_params(c) for c in part], outs, found)
            assert rc == 0, lib.peanut_last_error()
            got = found.cpu().tolist()
            for e, c in enumerate(part):
                assert got[e] == c["want_found"], (E, c["name"])
                assert np.array_equal(outs[e].cpu().numpy(), c["want"]), (E, c["name"])


def _view_in_parent(c, k):
    """The case's map as a view inside a larger tensor of other values; the parent's size and the offset depend on ``k``, so that
    the views of one batch differ from each other in plane stride, row stride and base address."""
    m = c["local_map"].shape[1]
    g = torch.Generator().manual_seed(50 + k)
    rows, cols = 2 * m + 3 * (k % 3), 2 * m + 5 * (k % 4)
    parent = (torch.rand((gmc.C, rows, cols), generator=g) * 0.5 + 0.25).cuda()
    r0, c0 = (3 + 7 * k) % (rows - m + 1), (m - 3 + 11 * k) % (cols - m + 1)
    view = parent[:, r0:r0 + m, c0:c0 + m]
    view.copy_(c["dev"])
    assert not view.is_contiguous()
    return parent, view, parent.clone()


@pytest.mark.parametrize("E", [3, 16])
def test_batches_mix_contiguous_maps_and_views_of_different_strides(lib, cases, E):
    """Episodes of one batch differ in their strides (in lock-step some episodes were rebound to their full map on the step,
    others not): every second episode is a view into a parent of its own size at its own offset, the others are contiguous, in
    both orders (episode 0 a view, then episode 0 contiguous).  Each episode equals the golden; no parent is written."""
    for m in (gmc.M, gmc.M_RANDOM):
        group = [c for c in cases if c["local_map"].shape[1] == m]
        for view_parity in (0, 1):
            for lo in range(0, len(group), E):
                part = group[lo:lo + E]
                if len(part) < E:
                    part = part + group[:E - len(part)][::-1]
                maps, parents = [], []
                for e, c in enumerate(part):
                    if e % 2 != view_parity:
                        maps.append(c["dev"])
                    else:
                        parent, view, before = _view_in_parent(c, lo + e)
                        maps.append(view)
                        parents.append((parent, before, c["name"]))
                strides = {(int(t.stride(0)), int(t.stride(1))) for t in maps}
                assert len(strides) >= 3 if E >= 4 else len(strides) >= 2
                outs = [torch.full((m, m), 9, dtype=torch.uint8, device="cuda") for _ in part]
                found = torch.full((E,), -1, dtype=torch.int32, device="cuda")
                rc = _batch(lib, maps, [_params(c) for c in part], outs, found)
                assert rc == 0, lib.peanut_last_error()
                got = found.cpu().tolist()
                for e, c in enumerate(part):
                    assert got[e] == c["want_found"], (E, view_parity, e, c["name"])
                    assert np.array_equal(outs[e].cpu().numpy(), c["want"]), (E, view_parity, e, c["name"])
                for parent, before, name in parents:
                    assert torch.equal(parent, before), name


def test_strided_view_into_a_larger_map_is_read_in_place(lib, cases):
    """The local map as a view at an offset inside a [C, 2m, 2m] tensor (Agent_State.local_map after update_full_map)."""
    for name in ("far_corner", "corner_4x4", "overlap_part", "random00", "random05"):
        c = next(x for x in cases if x["name"] == name)
        m = c["local_map"].shape[1]
        g = torch.Generator().manual_seed(5)
        # around the view: other values in every plane, which must not leak in (outside the map is set / unset by rule, not by memory)
        parent = (torch.rand((gmc.C, 2 * m, 2 * m), generator=g) * 0.5 + 0.25).cuda()
        r0, c0 = 7, m - 3
        view = parent[:, r0:r0 + m, c0:c0 + m]
        view.copy_(c["dev"])
        before = parent.clone()
        assert not view.is_contiguous()
        gm, found = _single(lib, view, _params(c))
        assert found == c["want_found"] and np.array_equal(gm, c["want"]), name
        assert torch.equal(parent, before), name


def test_the_same_output_buffers_over_three_calls(lib, cases):
    by = {c["name"]: c for c in cases}
    out = torch.zeros((gmc.M, gmc.M), dtype=torch.uint8, device="cuda")
    found = torch.zeros(1, dtype=torch.int32, device="cuda")
    for name in ("sq7_erode0", "sq6_vanishes", "sq7_across_32"):        # found, not found, found
        c = by[name]
        gm, f = _single(lib, c["dev"], _params(c), out=out, found=found)
        assert f == c["want_found"] and np.array_equal(gm, c["want"]), name


def test_refused_calls_write_nothing(lib, cases):
    from peanut_amd import _lib
    by = {c["name"]: c for c in cases}
    c = by["sq7_interior"]
    m = gmc.M
    maps = [c["dev"]] * 17
    outs = [torch.full((m, m), 9, dtype=torch.uint8, device="cuda") for _ in range(17)]
    found = torch.full((17,), -1, dtype=torch.int32, device="cuda")
    good = _params(c)

    def refused(rc):
        torch.cuda.synchronize()
        assert rc == -2, rc
        assert all(int(o.min()) == 9 and int(o.max()) == 9 for o in outs) and found.cpu().tolist() == [-1] * 17

    refused(_batch(lib, maps, [good] * 17, outs, found))                               # E = 17
    E = 3
    ptrs = (C.c_void_p * E)(c["dev"].data_ptr(), None, c["dev"].data_ptr())            # a null map
    ps = (C.c_longlong * E)(*[m * m] * E)
    rs = (C.c_longlong * E)(*[m] * E)
    pr = (C.c_int * (6 * E))(*(good * E))
    op = (C.c_void_p * E)(*[o.data_ptr() for o in outs[:E]])
    args = (int(c["dev"].shape[0]), m)
    refused(lib.peanut_goal_map_batch(E, ptrs, *args, ps, rs, pr, op, found.data_ptr(), _lib.current_stream_ptr()))
    ptrs = (C.c_void_p * E)(*[c["dev"].data_ptr()] * E)
    refused(lib.peanut_goal_map_batch(E, ptrs, *args, ps, rs, pr, op, None, _lib.current_stream_ptr()))      # null found
    shared = (C.c_void_p * E)(outs[0].data_ptr(), outs[1].data_ptr(), outs[0].data_ptr())
    refused(lib.peanut_goal_map_batch(E, ptrs, *args, ps, rs, pr, shared, found.data_ptr(), _lib.current_stream_ptr()))
    both = torch.full((2 * m * m - 1,), 9, dtype=torch.uint8, device="cuda")       # two goal maps that overlap in one byte
    overlap = (C.c_void_p * E)(outs[0].data_ptr(), both.data_ptr(), both.data_ptr() + m * m - 1)
    refused(lib.peanut_goal_map_batch(E, ptrs, *args, ps, rs, pr, overlap, found.data_ptr(), _lib.current_stream_ptr()))
    assert int(both.min()) == 9 and int(both.max()) == 9
    for k, bad in ((2, 9), (2, -1), (0, 3), (0, gmc.C), (4, m), (4, -1), (5, m), (1, 2), (3, 2)):
        # n_erode = 9 / -1, cn = 3 / channels, goal row / column out of range, morph / detect not 0 or 1 -- in the LAST episode
        p = [list(good) for _ in range(E)]
        p[E - 1][k] = bad
        refused(_batch(lib, maps[:E], p, outs[:E], found))
        single = torch.full((m, m), 9, dtype=torch.uint8, device="cuda")
        rc = lib.peanut_goal_map(c["dev"].data_ptr(), gmc.C, m, m * m, m, *p[E - 1], single.data_ptr(), found.data_ptr(),
                                 _lib.current_stream_ptr())
        torch.cuda.synchronize()
        assert rc == -2 and int(single.min()) == 9
    # rows that would overlap
    rc = lib.peanut_goal_map(c["dev"].data_ptr(), gmc.C, m, m * m, m - 1, *good, outs[0].data_ptr(), found.data_ptr(),
                             _lib.current_stream_ptr())
    refused(rc)


# ---------------------------------------------------------------- agent level ----------------------------------------------------------------

N_FRAMES = 10
LENGTHS = (10, 7, 10)
GOALS = (2, 5, 1)            # plant; tv_monitor (no erosion); sofa
LOCAL_STEPS = (3, 2, 3)      # num_local_steps per episode: local_map is a view into full_map on steps 2, 5, 8 / 1, 3, 5 / 2, 5, 8


class _FakePrediction:
    """Depends on the crop it is given (the formula of oracle.agent_ref.FakePrediction on HIP tensors)."""

    def __init__(self, size):
        from oracle.agent_ref import fake_pattern
        self.pattern = torch.from_numpy(fake_pattern(size=size)).cuda()

    def get_prediction_batch(self, maps, apply_sigmoid=True, out=None):
        return torch.tanh(maps[:, [0, 1, 4, 5, 6, 7]] + self.pattern[None]) * 0.5 + 0.5


def _args(**over):
    from oracle.agent_ref import agent_args
    # a 240-cell full map, 120-cell local map (the projection's window, local_w / 2 + vision_range, must fit into it: 48 cells of
    # vision); the local period (3) makes local_map a view into full_map on every third step
    base = dict(only_explore=0, map_size_cm=1200, vision_range=48, prediction_window=240, num_local_steps=3, update_goal_freq=4,
                select_goal=True, goal_map=True, goal_erode=3)
    base.update(over)
    return agent_args(**base)


def _frames(seed, n, goal):
    """Ready observations: nothing of the goal category in the first two frames, then a wide mask of it over the floor and the
    boxes; in frames 5 and 6 another category lies over the left part of it."""
    from oracle import mapping_scenes
    other = 5 if goal != 5 else 2
    out = []
    for i, fr in enumerate(mapping_scenes.make_sequence(seed=seed, n_frames=n)):
        sem = np.zeros_like(fr["sem"])
        if i >= 2:
            sem[goal, 40:118, 30:130] = 1
        if i in (5, 6):
            sem[other, 40:118, 20:90] = 1
        sem[7, 10:30, 100:150] = 1
        fr = dict(fr, sem=sem)
        out.append(dict(obs=torch.from_numpy(mapping_scenes.frame_to_obs(fr))[None].cuda(), sensor_pose=[float(v) for v in fr["pose"]]))
    return out


def _record(s):
    return dict(goal_map=None if s.goal_map is None else s.goal_map.cpu().numpy().copy(), found=s.found_goal,
                local_map=s.local_map.cpu().numpy().copy(), goals=[list(map(int, g)) for g in s.global_goals],
                view=not s.local_map.is_contiguous())


@pytest.fixture(scope="module")
def alone():
    """Each of the three episodes run by itself with the switch on: per step the goal map, found_goal, the local map and goal."""
    from peanut_amd.agent_state import Agent_State
    from peanut_amd.replay import run_episode
    args = _args()
    model = _FakePrediction(args.prediction_window)
    runs = []
    for e, (n, goal) in enumerate(zip(LENGTHS, GOALS)):
        st = Agent_State(_args(num_local_steps=LOCAL_STEPS[e]), prediction_model=model)
        steps = []
        run_episode(st, _frames(40 + e, n, goal), goal_cat=goal, on_step=lambda i, s, p, steps=steps: steps.append(_record(s)))
        runs.append((st, steps))
    return args, model, runs


def test_agent_goal_map_equals_the_reference_rule_on_every_step(alone):
    from peanut_amd.peanut_agent import coco_goal_names
    args, model, runs = alone
    for e, ((st, steps), goal) in enumerate(zip(runs, GOALS)):
        morph = int("tv" not in coco_goal_names[goal])
        assert len(steps) == LENGTHS[e]
        for i, r in enumerate(steps):
            want, want_found = gmc.goal_map_ref(r["local_map"], goal + 4, morph, 3, 1, r["goals"][0])
            print(f"episode {e} step {i}: found {r['found']} (reference rule {want_found}), cells {int(r['goal_map'].sum())}, "
                  f"goal {r['goals'][0]}, view {r['view']}")
            assert r["goal_map"].dtype == np.uint8 and r["goal_map"].shape == (st.local_w, st.local_h)
            assert r["found"] == want_found and np.array_equal(r["goal_map"], want), (e, i)
        assert any(r["view"] for r in steps) and not all(r["view"] for r in steps)     # both layouts of local_map were read
    found = [r["found"] for r in runs[0][1]]
    assert 0 in found and 1 in found, found                                            # the sequence shows both answers
    assert GOALS[1] == 5 and "tv" in coco_goal_names[5]


def test_the_switch_changes_no_map_state_and_off_leaves_goal_map_none(alone):
    from peanut_amd.agent_state import Agent_State
    from peanut_amd.replay import run_episode
    args, model, runs = alone
    st = Agent_State(_args(goal_map=False), prediction_model=model)
    seen = []
    run_episode(st, _frames(40, LENGTHS[0], GOALS[0]), goal_cat=GOALS[0], on_step=lambda i, s, p: seen.append(s.goal_map))
    assert seen == [None] * LENGTHS[0] and st.goal_map is None
    on = runs[0][0]
    assert torch.equal(st.local_map, on.local_map) and torch.equal(st.full_map, on.full_map)
    assert st.global_goals == on.global_goals and torch.equal(st.local_pose, on.local_pose)
    with pytest.raises(RuntimeError):
        st.planner_inputs({"goal_name": "plant"})


def test_planner_inputs_have_the_reference_dtypes_shapes_and_values(alone):
    args, model, runs = alone
    st = runs[0][0]
    infos = {"goal_name": "plant"}
    p = st.planner_inputs(infos)
    assert sorted(p) == ["exp_pred", "found_goal", "goal", "goal_name", "obstacle", "pose_pred"]
    m = st.local_w
    for k, ch in (("obstacle", 0), ("exp_pred", 1)):
        assert isinstance(p[k], np.ndarray) and p[k].dtype == np.float32 and p[k].shape == (m, m)
        assert np.array_equal(p[k], st.local_map[ch].cpu().numpy())
    assert p["goal"].dtype == np.float64 and p["goal"].shape == (m, m) and np.isin(p["goal"], (0.0, 1.0)).all()
    assert np.array_equal(p["goal"], st.goal_map.cpu().numpy().astype(np.float64)) and p["goal"].sum() >= 1
    assert p["pose_pred"].shape == (7,) and np.array_equal(p["pose_pred"], st.planner_pose_inputs)
    assert p["pose_pred"] is not st.planner_pose_inputs
    assert p["found_goal"] == st.found_goal and p["found_goal"] in (0, 1) and p["goal_name"] == "plant"
    d = st.planner_inputs(infos, host=False)
    assert sorted(d) == sorted(p)
    assert d["goal"].data_ptr() == st.goal_map.data_ptr() and d["goal"].dtype == torch.uint8
    assert d["obstacle"].data_ptr() == st.local_map[0].data_ptr() and d["exp_pred"].data_ptr() == st.local_map[1].data_ptr()
    assert d["pose_pred"] is st.planner_pose_inputs and d["found_goal"] == st.found_goal


@pytest.mark.parametrize("batch_predictions", [False, True])
def test_lockstep_goal_maps_go_through_one_call_per_step(alone, batch_predictions):
    """Three episodes of different lengths and goal categories (one a tv) in lock-step: the default path (the batched goal solve
    on the steps where two episodes predict, the plain path on the others) and batch_predictions."""
    from peanut_amd.agent_state import Agent_State, Agent_State_Group
    from peanut_amd.replay import run_episodes
    args, model, runs = alone
    states = [Agent_State(_args(num_local_steps=k), prediction_model=model) for k in LOCAL_STEPS]
    eps = [_frames(40 + e, n, goal) for e, (n, goal) in enumerate(zip(LENGTHS, GOALS))]
    seen = [[] for _ in states]
    groups = []
    real_init = Agent_State_Group.__init__

    layouts = []

    def on_step(i, act, predicted):
        layouts.append({s.local_map.is_contiguous() for s in act})
        for s in act:
            seen[states.index(s)].append(_record(s))

    def spy(self, *a, **k):
        real_init(self, *a, **k)
        groups.append(self)
    Agent_State_Group.__init__ = spy
    try:
        run_episodes(states, eps, GOALS, on_step=on_step, batch_predictions=batch_predictions)
    finally:
        Agent_State_Group.__init__ = real_init
    assert len(groups) == 1 and groups[0].goal_map_batches == max(LENGTHS)
    assert groups[0].goal_batches >= 1                       # the batched goal solve ran on some step
    # the episodes' local periods differ: on some steps one batch held contiguous maps AND views into full maps, on others one kind
    assert {True, False} in layouts and {True} in layouts
    for e, (st, steps) in enumerate(runs):
        assert len(seen[e]) == len(steps)
        for i, (a, b) in enumerate(zip(seen[e], steps)):
            assert np.array_equal(a["local_map"], b["local_map"]) and a["goals"] == b["goals"], (e, i)
            assert a["found"] == b["found"] and np.array_equal(a["goal_map"], b["goal_map"]), (e, i)


def test_peanut_agent_act_carries_the_planner_inputs():
    from oracle import mapping_scenes
    from peanut_amd.peanut_agent import PEANUT_Agent
    for on in (True, False):
        args = _args(goal_map=on)
        agent = PEANUT_Agent(args, prediction_model=_FakePrediction(args.prediction_window))
        agent.reset()
        for i, fr in enumerate(mapping_scenes.make_sequence(seed=3, n_frames=3)):
            out = agent.act({"gps": np.array([0.1 * i, 0.0], np.float32), "compass": np.array([0.0], np.float32),
                             "objectgoal": np.array([4]), "obs": torch.from_numpy(mapping_scenes.frame_to_obs(fr))[None]})
            assert ("planner_inputs" in out) == on
            if on:
                p = out["planner_inputs"]
                st = agent.agent_states
                assert p["goal_name"] == "tv_monitor" and p["found_goal"] == st.found_goal
                assert np.array_equal(p["goal"], st.goal_map.cpu().numpy().astype(np.float64))
                assert np.array_equal(p["pose_pred"], out["pose_pred"])
