"""The batched short-term goal on the device (peanut_stg_plan_batch, peanut_amd.planner.get_stg_batch,
Agent_State_Group.short_term_goals) against the SINGLE call, which tests/test_stg_gpu.py holds to the reference's own ``_get_stg``:
every episode's result struct and the taps of its last solve, bit for bit, at n = m + 2 = 64 (2 x 2 solver tiles exactly), 63 and 47
(ragged), for E = 1, 2, 3, 6 and 16, in other orders of the episodes, on handles with any history, and through the lock-step group."""
import ctypes as C
import itertools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stg_batch_cases as bc           # noqa: E402
import stg_cases as sc                 # noqa: E402
import workspace_cases as wc           # noqa: E402
from test_stg_gpu import _upload       # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("stg", "distance", "stop", "replan", "retried", "n_magnify", "n_solves", "trav", "goal", "dist")


def new_planner(c):
    from peanut_amd.planner import ShortTermGoal
    args = SimpleNamespace(map_size_cm=c["full"] * 5, map_resolution=5, global_downscaling=2, col_rad=c["col_rad"],
                           magnify_goal_when_hard=sc.MAGNIFY_WHEN_HARD)
    return ShortTermGoal(args, device="cuda:0")


_POOL = {}


def pool(c, n):
    """n planners of this case's group, kept for the module (no result depends on their history: that is tested below)."""
    have = _POOL.setdefault(bc.group_key(c), [])
    while len(have) < n:
        have.append(new_planner(c))
    return have[:n]


def inputs(c, view=False):
    return (c["obstacle_view"] if view else c["obstacle_dev"], c["goal_dev"], c["collision_dev"], c["visited_dev"], c["lmb"], c["start_exact"],
            c["found_goal"], c["goal_name"])


def single(c, p=None):
    p = p or pool(c, 1)[0]
    p.get_stg(*inputs(c), taps=True)
    return dict(p.last)


def batch(planners, cases, view=False, taps=True):
    from peanut_amd.planner import get_stg_batch
    got = get_stg_batch(planners, [inputs(c, view) for c in cases], taps=taps)
    for p, g in zip(planners, got):
        assert wc.same(g, (p.last["stg"], p.last["stop"]))
    return [dict(p.last) for p in planners]


@pytest.fixture(scope="module")
def groups():
    """Every group of stg_batch_cases and the sixteen variants, on the device, each case with its single-call result (computed once)."""
    g = {k: [_upload(c) for c in v] for k, v in bc.groups().items()}
    g["variants16"] = [_upload(c) for c in bc.variants16()]
    for cases in g.values():
        for c in cases:
            c["single"] = single(c)
            assert set(c["single"]) == set(KEYS)
    return g


def orders(E):
    if E <= 3:
        return list(itertools.permutations(range(E)))
    rot = [tuple((k + r) % E for k in range(E)) for r in range(0, E, max(1, E // 6))]
    return rot + [tuple(reversed(range(E))), tuple(range(0, E, 2)) + tuple(range(1, E, 2))]


@pytest.mark.parametrize("which,E", [(bc.FULL_GROUP, 1), (bc.PAIR_GROUP, 2), (bc.TRIPLE_GROUP, 3), (bc.FULL_GROUP, 6), ("variants16", 16)],
                         ids=["E1_n64", "E2_n63", "E3_n63", "E6_n64", "E16_n47"])
def test_every_episode_gets_the_bits_of_its_single_call_in_every_order(groups, which, E):
    cases = groups[which][:E] if E > 1 else [groups[which][1]]          # E = 1: serpentine_chair, nine solves
    assert len(cases) == E and cases[0]["m"] + 2 == {1: 64, 2: 63, 3: 63, 6: 64, 16: 47}[E]
    planners = pool(cases[0], E)
    for k, order in enumerate(orders(E)):
        view = k % 2 == 1                                                # every other order reads the obstacle as a strided view
        assert not view or not cases[0]["obstacle_view"].is_contiguous()
        got = batch(planners, [cases[e] for e in order], view=view)
        for slot, e in enumerate(order):
            assert wc.same(got[slot], cases[e]["single"]), (order, slot, cases[e]["name"], wc.first_difference(got[slot], cases[e]["single"]))
        # one synchronising wave per solve of the LONGEST chain, not per solve of the batch
        longest = max(c["single"]["n_solves"] for c in cases)
        assert [p.waves for p in planners] == [longest] * E
        assert E == 1 or longest < sum(c["single"]["n_solves"] for c in cases)
    for c in cases:
        assert torch.equal(c["obstacle_view"], c["obstacle_dev"])       # read in place, never written
    without = batch(planners, cases, taps=False)
    assert all(wc.same(g, {k: v for k, v in c["single"].items() if k not in ("trav", "goal", "dist")}) for g, c in zip(without, cases))


def test_the_flows_reached_cover_plain_retry_magnify_and_both(groups):
    flows = {c["name"]: (c["single"]["retried"], c["single"]["n_magnify"], c["single"]["n_solves"]) for cases in groups.values() for c in cases}
    print(flows)
    full = {c["name"]: flows[c["name"]] for c in groups[bc.FULL_GROUP]}
    assert full["serpentine_toilet"] == (0, 2, 3) and full["serpentine_chair"] == (0, 8, 9) and full["plugged_corridor"] == (1, 0, 2)
    assert full["plugged_serpentine"] == (1, 8, 10) and full["serpentine_shortcut"][:2] == (0, 2)
    assert len({f[2] for f in full.values()}) >= 4
    kinds = {(r, min(k, 1)) for r, k, _ in flows.values()}
    assert kinds == {(0, 0), (1, 0), (0, 1), (1, 1)}, kinds
    kinds16 = {(c["single"]["retried"], min(c["single"]["n_magnify"], 1)) for c in groups["variants16"]}
    assert kinds16 == {(0, 0), (1, 0)}, kinds16      # (no walk of a 45 x 45 map here is longer than 100 cells: plain and retried chains)


def test_two_identical_episodes_agree_with_each_other(groups):
    cases = groups[bc.FULL_GROUP]
    a, other = cases[4], cases[0]                                        # plugged_serpentine twice around serpentine_toilet
    got = batch(pool(a, 3), [a, other, a])
    assert wc.same(got[0], got[2]) and got[0]["trav"].data_ptr() != got[2]["trav"].data_ptr()
    assert wc.same(got[0], a["single"]) and wc.same(got[1], other["single"])


def test_results_do_not_depend_on_the_handles_history(groups):
    cases = groups[bc.FULL_GROUP]
    want = [c["single"] for c in cases]
    E = len(cases)

    def check(got, what, order=None):
        for slot, e in enumerate(order or range(E)):
            assert wc.same(got[slot], want[e]), (what, cases[e]["name"], wc.first_difference(got[slot], want[e]))
    fresh = [new_planner(cases[0]) for _ in range(E)]
    check(batch(fresh, cases), "fresh handles")
    with wc.poisoned():
        poisoned = [new_planner(cases[0]) for _ in range(E)]
        check(batch(poisoned, cases), "poisoned handles")
        check(batch(poisoned, cases), "poisoned handles, second call")
    # used before in another order (every handle then holds another episode's masks, field and round hints; another handle led)
    rev = list(reversed(range(E)))
    check(batch(fresh, [cases[e] for e in rev]), "reversed", rev)
    check(batch(fresh, cases), "after the reversed batch")
    check(batch(fresh[1:] + fresh[:1], cases), "handles rotated: another one leads")
    check(batch(fresh, cases), "after the rotated batch")
    # single calls in between, on the lead and on a member
    single(cases[1], fresh[0])
    single(cases[0], fresh[3])
    check(batch(fresh, cases), "after single calls")
    assert wc.same(single(cases[2], fresh[2]), want[2])                  # ... and the single call after a batch
    # after a refused call
    from peanut_amd import _lib
    from peanut_amd.planner import get_stg_batch
    bad = [list(inputs(c)) for c in cases]
    bad[3][5] = [-0.5, 3.0]
    with pytest.raises(_lib.PeanutHipError):
        get_stg_batch(fresh, bad)
    check(batch(fresh, cases), "after a refused call")


def _descriptor(planners, cases, results, taps, **over):
    """A raw peanut_stg_batch_t over these episodes; ``over``: field -> replacement value (arrays are kept alive in the tuple)."""
    from peanut_amd import _lib
    E = len(planners)
    ptr = lambda vals: (C.c_void_p * len(vals))(*vals)                   # noqa: E731
    f = dict(h=ptr([p._h.value for p in planners]), obstacle=ptr([c["obstacle_dev"].data_ptr() for c in cases]),
             row_stride=(C.c_longlong * E)(*[c["m"] for c in cases]), goal_map=ptr([c["goal_dev"].data_ptr() for c in cases]),
             collision=ptr([c["collision_dev"].data_ptr() for c in cases]), visited=ptr([c["visited_dev"].data_ptr() for c in cases]),
             lmb=(C.c_int * (4 * E))(*[v for c in cases for v in c["lmb"]]),
             start_exact=(C.c_double * (2 * E))(*[v for c in cases for v in c["start_exact"]]),
             found_goal=(C.c_int * E)(*[c["found_goal"] for c in cases]), radius_found=(C.c_int * E)(*[8] * E),
             magnify_when_hard=(C.c_double * E)(*[100.0] * E), max_magnify=(C.c_int * E)(*[8] * E), result_out=results,
             trav_out=ptr([t[0].data_ptr() for t in taps]), goal_out=ptr([t[1].data_ptr() for t in taps]),
             dist_out=ptr([t[2].data_ptr() for t in taps]), stream=_lib.current_stream_ptr(), size=C.sizeof(_lib.StgBatchC), E=E, reserved=0)
    f.update(over)
    return _lib.StgBatchC(**f), f


def test_batch_refuses_bad_arguments_before_anything_is_enqueued(groups):
    from peanut_amd import _lib
    lib = _lib.load()
    cases = groups[bc.TRIPLE_GROUP]
    E, m, full, n = 3, cases[0]["m"], cases[0]["full"], cases[0]["m"] + 2
    planners = [new_planner(cases[0]) for _ in range(E)]
    taps = [[torch.full((n, n), 0x5A, dtype=torch.uint8, device="cuda"), torch.full((n, n), 0x5A, dtype=torch.uint8, device="cuda"),
             torch.full((n, n), -7.0, dtype=torch.float64, device="cuda")] for _ in range(E)]
    keep = [[t.clone() for t in tap] for tap in taps]
    handles = {}
    for name, a in dict(small=(9, 18, 18, 0, 5), wide=(m, full, full, 17, 5), other_m=(m - 1, full, full, 0, 5), other_full_w=(m, full + 2, full, 0, 5),
                        other_full_h=(m, full, full + 2, 0, 5), other_rad=(m, full, full, 1, 5), other_step=(m, full, full, 0, 4)).items():
        handles[name] = C.c_void_p()
        _lib.check(lib.peanut_stg_create(C.byref(handles[name]), *a), "peanut_stg_create")
    hs = [p._h.value for p in planners]
    ptr = lambda vals: (C.c_void_p * len(vals))(*vals)                   # noqa: E731

    def call(name, use=None, **over):
        res = (_lib.StgResultC * E)()
        C.memset(res, 0x6B, C.sizeof(res))
        before = bytes(res)
        d, alive = _descriptor(planners, use or cases, res, taps, **over)
        rc = lib.peanut_stg_plan_batch(C.byref(d))
        torch.cuda.synchronize()
        assert rc == -2, (name, rc, lib.peanut_last_error())
        assert bytes(res) == before, name
        assert all(torch.equal(t, k) for tap, kp in zip(taps, keep) for t, k in zip(tap, kp)), name

    def at(field, e, value, per=1):
        """The episode arrays with entry e of ``field`` replaced."""
        _, f = _descriptor(planners, cases, None, taps)
        arr = f[field]
        for k, v in enumerate(value if per > 1 else [value]):
            arr[per * e + k] = v
        return {field: arr}
    size = C.sizeof(_lib.StgBatchC)
    call("size_small", size=size - 8)
    call("size_large", size=size + 8)
    call("size_zero", size=0)
    call("E_zero", E=0)
    call("E_17", E=17)
    call("E_negative", E=-1)
    for field in ("h", "obstacle", "row_stride", "goal_map", "collision", "visited", "lmb", "start_exact", "found_goal", "radius_found",
                  "magnify_when_hard", "max_magnify", "result_out"):
        call(f"null_array_{field}", **{field: None})
    for field in ("h", "obstacle", "goal_map", "collision", "visited"):
        call(f"null_entry_{field}", **at(field, 1, None))
    call("same_handle_twice", h=ptr([hs[0], hs[1], hs[0]]))
    for name in ("other_m", "other_full_w", "other_full_h", "other_rad", "other_step"):
        call(name, h=ptr([hs[0], hs[1], handles[name].value]))
    gx1, gx2, gy1, gy2 = cases[2]["lmb"]
    call("lmb_size", **at("lmb", 2, [gx1, gx2 - 1, gy1, gy2], 4))
    call("lmb_outside", **at("lmb", 2, [gx1 + full, gx2 + full, gy1, gy2], 4))
    call("lmb_negative", **at("lmb", 0, [-1, m - 1, gy1, gy2], 4))
    call("start_negative", **at("start_exact", 1, [-0.25, 5.0], 2))
    call("start_beyond", **at("start_exact", 2, [5.0, float(m)], 2))
    call("start_nan", **at("start_exact", 0, [float("nan"), 5.0], 2))
    found = {c["name"]: c["found_goal"] for c in cases}
    e_found = next((e for e, c in enumerate(cases) if c["found_goal"] == 1), None)
    if e_found is None:
        call("radius", found_goal=(C.c_int * E)(1, 1, 1), **at("radius_found", 1, 17))
    else:
        call("radius", **at("radius_found", e_found, 17))
    call("stride", **at("row_stride", 1, m - 1))
    # handles of one kind that the single call refuses as well: m < 2 step_size + 1, col_rad above the limit
    for name, args in (("small", (9, 18, 18, 0, 5)), ("wide", (m, full, full, 17, 5))):
        more = [C.c_void_p(), C.c_void_p()]
        for h in more:
            _lib.check(lib.peanut_stg_create(C.byref(h), *args), "peanut_stg_create")
        over = dict(h=ptr([handles[name].value, more[0].value, more[1].value]))
        if name == "small":
            over.update(lmb=(C.c_int * 12)(*[0, 9, 0, 9] * 3), start_exact=(C.c_double * 6)(*[4.0, 4.0] * 3), row_stride=(C.c_longlong * 3)(9, 9, 9))
        call(f"all_{name}", **over)
        for h in more:
            lib.peanut_stg_destroy(h)
    assert found                                                          # (the cases were read)
    got = batch(planners, cases)                                          # the handles that refused all of these still plan
    assert all(wc.same(g, c["single"]) for g, c in zip(got, cases))
    for h in handles.values():
        lib.peanut_stg_destroy(h)


def test_python_refuses_empty_oversized_and_mixed_batches(groups):
    from peanut_amd.planner import MAX_BATCH, get_stg_batch
    cases = groups[bc.PAIR_GROUP]
    a, b = pool(cases[0], 2)
    with pytest.raises(ValueError):
        get_stg_batch([], [])
    other = groups[bc.TRIPLE_GROUP][0]
    with pytest.raises(ValueError):
        get_stg_batch([a, pool(other, 1)[0]], [inputs(cases[0]), inputs(other)])            # mixed: another col_rad
    with pytest.raises(ValueError):
        get_stg_batch([a, a], [inputs(cases[0]), inputs(cases[1])])
    with pytest.raises(ValueError):
        get_stg_batch([a, b], [inputs(cases[0])])
    with pytest.raises(ValueError):
        get_stg_batch([a] * (MAX_BATCH + 1), [inputs(cases[0])] * (MAX_BATCH + 1))
    bad = list(inputs(cases[1]))
    bad[1] = bad[1].to(torch.float32)
    single(cases[0], a)
    last = dict(a.last)
    with pytest.raises(ValueError):
        get_stg_batch([a, b], [inputs(cases[0]), bad])                                       # the single call's tensor checks, per episode
    assert wc.same(dict(a.last), last)
    got = batch([a, b], cases)
    assert all(wc.same(g, c["single"]) for g, c in zip(got, cases))


# ---- the lock-step group ----
def test_group_short_term_goals_equal_each_states_own_in_lock_step():
    """Three episodes of test_lockstep_gpu._episodes() (12, 9 and 12 frames) with goal_map and plan_stg on: after every step the
    group's batched short-term goals equal each state's own short_term_goal bit for bit, also after the 9-frame episode dropped out;
    stg_batches counts with batch_stg on and stays 0 with it off, and both runs leave the same goals."""
    import test_lockstep_gpu as tl
    from oracle.agent_ref import agent_args
    from peanut_amd.agent_state import Agent_State
    from peanut_amd.peanut_agent import coco_goal_names
    from peanut_amd.prediction import PEANUT_Prediction_Model
    from peanut_amd.replay import run_episodes
    from peanut_amd.weights import PredCfg, make_seeded_state_dict
    args = agent_args(only_explore=0, prediction_window=240, map_size_cm=2400, select_goal=True, num_local_steps=5, goal_map=True,
                      goal_erode=3, plan_stg=True)
    model = PEANUT_Prediction_Model(args, state_dict=make_seeded_state_dict(PredCfg(), 0))
    eps, goals = tl._episodes(), tl.GOALS

    def scenario(batch_stg):
        states = [Agent_State(args, prediction_model=model) for _ in range(3)]
        holder, steps = [], []

        def on_step(i, act, predicted):
            group = holder[0]
            infos = [{"goal_name": coco_goal_names.get(int(goals[states.index(s)]), "")} for s in act]
            got = group.short_term_goals(infos)
            assert got == [(s.stg, s.stg_stop) for s in act]
            lasts = [dict(s._stg.last) for s in act]
            for s, info, g, last in zip(act, infos, got, lasts):
                own = s.short_term_goal(info)
                assert wc.same(own, g) and wc.same(dict(s._stg.last), last), (i, states.index(s), last, s._stg.last)
            steps.append((got, lasts))
        n = run_episodes(states, eps, goals, on_step=on_step, on_group=holder.append, batch_stg=batch_stg)
        return holder[0], n, steps
    group, n, steps = scenario(True)
    assert [len(s[0]) for s in steps] == [3] * 9 + [2] * 3 and all(c >= 1 for c in n)
    assert group.stg_batches == 12 and group.batch_stg
    off, n_off, steps_off = scenario(False)
    assert off.stg_batches == 0 and not off.batch_stg and n_off == n
    assert wc.same(steps, steps_off)
    # a subset, and an episode with plan_stg off, go where they belong
    act = list(group.states)
    group.reset_active()
    infos = [{"goal_name": coco_goal_names.get(int(g), "")} for g in goals]
    before = group.stg_batches
    one = group.short_term_goals(infos[2:], states=act[2:])
    assert group.stg_batches == before and wc.same(one[0], act[2].short_term_goal(infos[2]))
    with pytest.raises(ValueError):
        group.short_term_goals(infos[:1])
