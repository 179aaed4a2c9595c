"""The stream contract of peanut_stg_plan_batch, class "syncs": the call is ordered behind whatever is in flight on the caller's stream
(its inputs may be written by work enqueued just before it) and has read every input when it returns (they may be overwritten right
after it).  Its stream travels in the descriptor, where the prototype check of tests/test_streams_cpu.py does not see it, so the row
the contract table owes it is held here, with the protocols of tests/stream_cases.py: P1 (late input, early overwrite) and P2 (back to
back on fresh handles) at E = 3 on the scenes of ``stream_cases.stg_scenes``, and the lock-step scenario of tests/test_streams_gpu.py
with the group's batched short-term goals in ``on_step``, plain against a side stream with a backlog before every step."""
import os
import re
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_cases as sc              # noqa: E402

pytestmark = pytest.mark.gpu

CLASS = "syncs"
E = 3


def test_the_header_says_that_the_batch_call_synchronises():
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "peanut_hip.h"), encoding="utf-8") as f:
        src = f.read()
    comment = re.findall(r"/\*(.*?)\*/\s*#define PEANUT_STG_MAX_BATCH", src, flags=re.S)[-1]
    assert "peanut_stg_plan_batch" not in sc.CONTRACT          # (the table cannot see it; when it can, this file's row moves there)
    assert re.search(r"\bSynchronises\b", comment) and "descriptor" in comment


def _inputs(seeds):
    """E episodes' maps, flat: (obstacle, goal, collision, visited) of stg_scenes(seed) for each seed."""
    return [t for seed in seeds for t in sc.to_device(sc.stg_scenes(seed))]


def test_batched_plan_late_input_and_back_to_back():
    import stg_cases
    from peanut_amd.planner import ShortTermGoal, get_stg_batch
    c = next(s for s in stg_cases.scene_cases() if s["name"] == "blocked_start")
    args = SimpleNamespace(map_size_cm=c["full"] * 5, map_resolution=5, global_downscaling=2, col_rad=c["col_rad"],
                           magnify_goal_when_hard=stg_cases.MAGNIFY_WHEN_HARD)
    make = lambda: [ShortTermGoal(args, device="cuda:0") for _ in range(E)]  # noqa: E731

    def run(planners, x, outs):
        get_stg_batch(planners, [(x[4 * e], x[4 * e + 1], x[4 * e + 2], x[4 * e + 3], c["lmb"], c["start_exact"], c["found_goal"], c["goal_name"])
                                 for e in range(E)], taps=True)
        return [dict(p.last) for p in planners]
    good, stale = _inputs((0, 1, 2)), _inputs((1, 2, 0))
    planners = sc.p1("peanut_stg_plan_batch", make, run, good, stale, CLASS)
    got = run(planners, good, None)
    assert got[0]["retried"] == 1 and got[0]["n_solves"] >= 2 and planners[0].waves == max(g["n_solves"] for g in got)
    sc.p2("peanut_stg_plan_batch", make, run, [good, stale, _inputs((2, 0, 1))])


def test_lockstep_short_term_goals_behind_a_backlog_before_every_step():
    """test_lockstep_episodes_behind_a_backlog_before_every_step (E = 2, 12 and 9 frames, goal_map and plan_stg on) with the group's
    short_term_goals -- one peanut_stg_plan_batch per step while both episodes run -- in on_step."""
    import test_lockstep_gpu as tl
    import test_streams_gpu as ts
    from peanut_amd.agent_state import Agent_State
    from peanut_amd.peanut_agent import coco_goal_names
    from peanut_amd.replay import run_episodes
    args, model = ts._agent_setup(True)
    eps, goals = tl._episodes()[:2], tl.GOALS[:2]

    def scenario(before_step):
        states, steps, holder = [Agent_State(args, prediction_model=model) for _ in range(2)], [], []

        def on_step(i, act, predicted):
            infos = [{"goal_name": coco_goal_names.get(int(goals[states.index(s)]), "")} for s in act]
            got = holder[0].short_term_goals(infos)
            steps.append([dict(ts._record(s, goals[states.index(s)], p, False), stg=tuple(float(v) for v in g[0]), stop=bool(g[1]),
                               last=dict(s._stg.last)) for s, p, g in zip(act, predicted, got)])
            before_step()
        before_step()
        n = run_episodes(states, eps, goals, on_step=on_step, on_group=holder.append)
        return [n, steps, holder[0].stg_batches]
    plain, got = ts._in_a_backlogged_stream(scenario)
    assert all(c >= 1 for c in plain[0]) and [len(s) for s in plain[1]] == [2] * 9 + [1] * 3
    assert plain[2] == 9 == got[2]                              # batched while two episodes ran, single for the last three steps
    for i, (a, b) in enumerate(zip(got[1], plain[1])):
        sc.assert_same(a, b, f"step {i}")
    assert got[0] == plain[0]
