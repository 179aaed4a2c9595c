"""``peanut_amd.agent_helper.Agent_Helper`` against the reference's own ``_plan`` (tests/golden/plan_golden.npz, written by
tools/gen_golden_plan.py from the chains of tests/plan_cases.py).

1. Every chain through ``plan_act`` with the scripted short-term goal injected: after every step the action, every counter and
   both device maps equal the reference's, bit for bit.
2. The same chains as lock-step batches of E = 3 (``plan_act_batch``: one ``peanut_plan_mark_batch`` per step) against the same
   fixture, which is what single calls give; an episode whose chain has ended is simply not in the batch.
3. On the whole scenes of stg_golden.npz one full ``plan_act`` goes through the real device ``_get_stg``: the action equals the
   one the golden ``(stg, stop)`` implies, and the retry scene moves on to the next preset goal under ``only_explore``.
4. ``PEANUT_Agent`` with ``args.plan_act``: the switch, its ``ValueError``, and the ``'action'`` key.
5. ``Agent_State_Group.plan_acts`` on three lock-step episodes (real maps, real batched short-term goals) against single
   ``plan_act`` calls: actions, counters and maps bit for bit, also after the shortest episode dropped out."""
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import plan_cases as pc
import plan_world as pw
import stg_cases as sc
from peanut_amd.agent_helper import Agent_Helper, plan_act_batch

pytestmark = pytest.mark.gpu

CHAINS = pc.chains()


@pytest.fixture(scope="module")
def golden():
    return pc.load_golden()


def _helper(chain):
    args = SimpleNamespace(**pc.cfg_args(chain["cfg"]))
    state = pw.state_stand_in(args)
    h = Agent_Helper(args, state)
    h.reset()
    return h, state


def _inputs(chain, k):
    s, m = chain["steps"][k], pc.local_size(chain["cfg"])
    return {'obstacle': torch.zeros((m, m), device="cuda:0"), 'goal': torch.zeros((m, m), dtype=torch.uint8, device="cuda:0"),
            'pose_pred': np.array(list(s["pose"]) + s["lmb"], np.float64), 'found_goal': s["found"], 'goal_name': 'chair'}


def _row(h, action):
    return [action, h.col_width, h.prev_blocked, h.forward_after_stop, h._previous_action, h.last_action, h.untrap.total_id, h.untrap.epi_id,
            h.timestep, h.last_start[0], h.last_start[1]]


def _check(name, k, h, state, action, g):
    assert _row(h, action) == [int(v) for v in g["state"][k, :11]], (name, k, dict(zip(pc.STATE, _row(h, action))))
    vis, col = state.visited_vis.cpu().numpy(), state.collision_map.cpu().numpy()
    assert np.array_equal(vis, g["visited"][k]), f"{name} step {k}: visited_vis differs at {np.argwhere(vis != g['visited'][k])[:6].tolist()}"
    assert np.array_equal(col, g["collision"][k]), f"{name} step {k}: collision_map differs at {np.argwhere(col != g['collision'][k])[:6].tolist()}"


@pytest.mark.parametrize("name", sorted(CHAINS))
def test_every_chain_equals_the_reference_step_by_step(name, golden):
    chain, g = CHAINS[name], golden[name]
    h, state = _helper(chain)
    np.random.seed(chain["cfg"]["seed"])
    for k, s in enumerate(chain["steps"]):
        h._get_stg = lambda planner_inputs, step, s=s: (s["stg"], bool(s["stop"]))
        out = h.plan_act(_inputs(chain, k))
        assert set(out) == {'action'}
        _check(name, k, h, state, out['action'], g)
    assert h.collision_map is state.collision_map and h.visited_vis is state.visited_vis
    h.reset()
    assert int(state.collision_map.sum()) == 0 and int(state.visited_vis.sum()) == 0 and h.timestep == 0 and h.last_action is None


@pytest.mark.parametrize("names", [("walk_edges", "thresholds", "window_moves"), ("blocked", "stop1", "angles"), ("stop2", "stop0", "blocked")])
def test_lock_step_batches_equal_single_calls(names, golden):
    """Three chains of one window size side by side; the shorter ones drop out as they end.  The untrap's draws from the global RNG
    come in episode order, as in single calls: ``blocked`` is the only chain that draws, so its seed holds."""
    chains = [CHAINS[n] for n in names]
    made = [_helper(c) for c in chains]
    np.random.seed(CHAINS["blocked"]["cfg"]["seed"])
    for k in range(max(len(c["steps"]) for c in chains)):
        live = [e for e, c in enumerate(chains) if k < len(c["steps"])]
        script = lambda helpers, inputs, steps, live=live, k=k: [(chains[e]["steps"][k]["stg"], bool(chains[e]["steps"][k]["stop"])) for e in live]
        outs = plan_act_batch([made[e][0] for e in live], [_inputs(chains[e], k) for e in live], stg_batch=script)
        for e, out in zip(live, outs):
            _check(names[e], k, made[e][0], made[e][1], out['action'], golden[names[e]])


def test_batch_refuses_what_it_cannot_hold():
    h, _ = _helper(CHAINS["angles"])
    other, _ = _helper(CHAINS["border"])
    with pytest.raises(ValueError):
        plan_act_batch([h, h], [_inputs(CHAINS["angles"], 0)] * 2)
    with pytest.raises(ValueError):
        plan_act_batch([h], [])
    with pytest.raises(ValueError):
        plan_act_batch([], [])
    assert h.timestep == 0 and other.timestep == 0


# ---- one full plan_act through the real device _get_stg -------------------------------------------------------------------------
SCENE_RES = 25      # cm per cell in the scene test: a cell k / 4 is then the metric coordinate k / 16, exact in binary


def _pose_for(cell_exact, g0):
    """The metric coordinate v with ``v * 100.0 / SCENE_RES - g0 == cell_exact`` exactly (agent_helper.py:265-266).  With the
    reference's 5 cm cells no double gives the scenes' x.5 and x.25 cells in a window at 0 (1.025 * 100 / 5 = 20.499999999999996),
    and a start that is off in the last bit flips the window-mask cells that sit exactly on the circle."""
    v = np.float64((cell_exact + g0) * SCENE_RES / 100.0)
    assert v * 100.0 / SCENE_RES - g0 == cell_exact
    return float(v)


def _implied_action(stg, stop, found, start, heading, m, edge_buffer=10, turn_angle=30):
    """agent_helper.py:335-363 on a fresh helper (move_forward_after_stop = 1, nothing blocked)."""
    if stop and found == 1:
        return 1
    x = min(max(stg[0], edge_buffer), m - edge_buffer - 1)
    y = min(max(stg[1], edge_buffer), m - edge_buffer - 1)
    goal = math.degrees(math.atan2(x - start[0], y - start[1]))
    agent = heading % 360.0
    agent = agent - 360 if agent > 180 else agent
    rel = (agent - goal) % 360.0
    rel = rel - 360 if rel > 180 else rel
    return 3 if rel > turn_angle / 2. else 2 if rel < -turn_angle / 2. else 1


@pytest.mark.parametrize("case", sc.scene_cases(), ids=lambda c: c["name"])
def test_whole_scenes_give_the_action_the_golden_short_term_goal_implies(case):
    z = np.load(sc.GOLDEN)
    res = z[f"c/{case['name']}/result"]
    stg, stop, retried = (float(res[0]), float(res[1])), bool(res[2]), int(res[3])
    m, full = case["m"], case["full"]
    for heading, only_explore in ((0.0, 1), (135.0, 0)):
        args = SimpleNamespace(map_size_cm=full * SCENE_RES, map_resolution=SCENE_RES, global_downscaling=2, num_sem_categories=10, col_rad=case["col_rad"],
                               only_explore=only_explore, move_forward_after_stop=1, turn_angle=30, collision_threshold=0.20,
                               magnify_goal_when_hard=case.get("magnify_when_hard", sc.MAGNIFY_WHEN_HARD))
        state = pw.state_stand_in(args)
        h = Agent_Helper(args, state)
        h.reset()
        state.collision_map.copy_(torch.from_numpy(case["collision"]))       # (after reset, which zeroes them)
        state.visited_vis.copy_(torch.from_numpy(case["visited"]))
        gx1, gx2, gy1, gy2 = case["lmb"]
        y, x = _pose_for(case["start_exact"][0], gx1), _pose_for(case["start_exact"][1], gy1)
        h.curr_loc = [x, y, heading]                                           # the agent stood here before: the line is a point
        inputs = {'obstacle': torch.from_numpy(case["obstacle"]).cuda(), 'goal': torch.from_numpy(case["goal"]).cuda(),
                  'pose_pred': np.array([x, y, heading, gx1, gx2, gy1, gy2], np.float64), 'found_goal': case["found_goal"], 'goal_name': case["goal_name"]}
        visited = case["visited"].copy()
        start = [int(case["start_exact"][0]), int(case["start_exact"][1])]
        action = h.plan_act(inputs)['action']
        assert h.stg == stg and state.stg == stg and bool(state.stg_stop) == stop, (case["name"], h.stg, stg)
        assert action == _implied_action(stg, stop, case["found_goal"], start, heading, m), (case["name"], heading)
        assert state.presets == (retried if only_explore else 0)
        # the mark of this step: the point's 2 x 2 block, and nothing in the collision map
        visited[gx1:gx2, gy1:gy2][start[0] - 1:start[0] + 1, start[1] - 1:start[1] + 1] = 1
        assert np.array_equal(state.visited_vis.cpu().numpy(), visited) and np.array_equal(state.collision_map.cpu().numpy(), case["collision"])


# ---- the public switch ----------------------------------------------------------------------------------------------------------
def test_peanut_agent_returns_an_action_with_the_switch_on_and_needs_its_inputs():
    from oracle import mapping_scenes
    from peanut_amd.agent_state import default_args
    from peanut_amd.peanut_agent import PEANUT_Agent
    for bad in (dict(plan_act=True), dict(plan_act=True, goal_map=True), dict(plan_act=True, plan_stg=True)):
        with pytest.raises(ValueError):
            PEANUT_Agent(default_args(only_explore=1, **bad))
    d = default_args()
    assert (d.plan_act, d.turn_angle, d.collision_threshold, d.move_forward_after_stop) == (False, 30, 0.20, 1)
    outs = {}
    for on in (False, True):
        agent = PEANUT_Agent(default_args(only_explore=1, goal_map=True, plan_stg=True, plan_act=on))
        assert (agent.agent_helper is not None) == on
        agent.reset()
        outs[on] = []
        for i, fr in enumerate(mapping_scenes.make_sequence(seed=3, n_frames=4)):
            out = agent.act({"gps": np.array([0.1 * i, 0.0], np.float32), "compass": np.array([0.0], np.float32), "objectgoal": np.array([4]),
                             "obs": torch.from_numpy(mapping_scenes.frame_to_obs(fr))[None]})
            assert ('action' in out) == on
            outs[on].append(out)
        st = agent.agent_states
        if on:
            assert agent.agent_helper.collision_map is st.collision_map and agent.agent_helper.visited_vis is st.visited_vis
            assert int(st.visited_vis.sum()) > 0 and agent.agent_helper.timestep == 4 and st.helper is agent.agent_helper
            assert all(o['action'] in (0, 1, 2, 3) for o in outs[on])
            agent.reset()
            assert int(st.visited_vis.sum()) == 0 and agent.agent_helper.timestep == 0
        else:
            assert int(st.visited_vis.sum()) == 0 and int(st.collision_map.sum()) == 0
    # with the switch off the keys are what they were
    assert set(outs[False][0]) == {'predicted', 'sensor_pose', 'goal_name', 'pose_pred', 'global_goals', 'planner_inputs', 'stg', 'stop'}
    assert set(outs[True][0]) == set(outs[False][0]) | {'action'}
    # step 0: the first visited mark is the start's own block, which the short-term goal sets traversible anyway: same goal both ways
    assert outs[True][0]['stg'] == outs[False][0]['stg'] and outs[True][0]['stop'] == outs[False][0]['stop']


# ---- the lock-step group --------------------------------------------------------------------------------------------------------
def test_group_plan_acts_equal_single_plan_act_calls_in_lock_step():
    import test_lockstep_gpu as tl
    from oracle.agent_ref import agent_args
    from peanut_amd.agent_state import Agent_State
    from peanut_amd.replay import run_episodes
    args = agent_args(only_explore=1, map_size_cm=2400, num_local_steps=5, goal_map=True, goal_erode=3, plan_stg=True, plan_act=True,
                      turn_angle=30, collision_threshold=0.20, move_forward_after_stop=1, magnify_goal_when_hard=100)
    eps, goals = tl._episodes(), tl.GOALS

    def scenario(batched):
        states = [Agent_State(args) for _ in range(3)]
        helpers = [Agent_Helper(args, s) for s in states]
        for h in helpers:
            h.reset()
        holder, steps = [], []
        np.random.seed(11)

        def on_step(i, act, predicted):
            from peanut_amd.peanut_agent import coco_goal_names
            infos = [{"goal_name": coco_goal_names.get(int(goals[states.index(s)]), "")} for s in act]
            if batched:
                outs = holder[0].plan_acts(infos)
            else:
                outs = [s.helper.plan_act(s.planner_inputs(info, host=False)) for s, info in zip(act, infos)]
            steps.append([(o['action'], _row(s.helper, o['action']), s.stg, s.stg_stop, s.global_goal_preset_id) for s, o in zip(act, outs)])
        run_episodes(states, eps, goals, on_step=on_step, on_group=holder.append)
        for h in helpers:                    # (run_episodes resets the states, which zeroes the maps the helpers share with them)
            assert h.collision_map is h.agent_states.collision_map
        maps = [(s.visited_vis.cpu().numpy(), s.collision_map.cpu().numpy()) for s in states]
        return holder[0], steps, maps
    group, steps, maps = scenario(True)
    assert [len(s) for s in steps] == [3] * 9 + [2] * 3 and group.plan_batches == 12
    _, steps_single, maps_single = scenario(False)
    assert steps == steps_single
    for (v, c), (v1, c1) in zip(maps, maps_single):
        assert np.array_equal(v, v1) and np.array_equal(c, c1) and v.sum() > 0
    with pytest.raises(ValueError):
        group.plan_acts([{"goal_name": "chair"}])
