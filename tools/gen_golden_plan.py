"""Writes tests/golden/plan_golden.npz: what the reference's OWN ``Agent_Helper.plan_act`` / ``_plan`` / ``reset`` and
``UnTrapHelper`` (nav/agent/agent_helper.py:19-48, :106-159, :228-371) give on the chains of tests/plan_cases.py.

The reference's agent/agent_helper.py is imported at run time, unmodified, under the stand-in modules of tools/gen_golden_stg.py
(``load_reference``).  ``reset`` and ``plan_act`` are called unbound on a stand-in object that carries the fields ``__init__`` would
have set; its ``_get_stg`` is a script that returns the step's ``(stg, stop)``, so no solver arithmetic enters and every number in
the file is exact.  The global NumPy RNG is seeded per chain (the untrap sequence draws from it past 30 tries).

Per chain and step the file holds one ``state`` row (the columns of ``plan_cases.STATE``: the action, every counter, ``last_start``
and the number of set cells of either map) and the two maps after the step as uint8 [T, 96, 96]: numeric arrays only.

Needs the reference checkout (it does not travel with the tests; the .npz does).

    python -m tools.gen_golden_plan
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import plan_cases as pc                              # noqa: E402
from tools.gen_golden_stg import load_reference      # noqa: E402


def run_chain(ah, chain):
    """The reference's ``reset`` and then ``plan_act`` per step on a stand-in -> (state [T, len(STATE)], visited, collision)."""
    cfg = chain["cfg"]
    args = types.SimpleNamespace(**pc.cfg_args(cfg))
    m = pc.local_size(cfg)
    script = {}
    me = types.SimpleNamespace(args=args, untrap=ah.UnTrapHelper(), episode_no=0, last_action=None, stg=None, goal_cat=-1,
                               forward_after_stop_preset=args.move_forward_after_stop, forward_after_stop=args.move_forward_after_stop,
                               full_w=pc.FULL, full_h=pc.FULL, local_w=m, local_h=m, edge_buffer=10 if args.num_sem_categories <= 16 else 40)
    me._get_stg = lambda grid, start, goal, window: (script["stg"], script["stop"])
    me._plan = lambda planner_inputs: ah.Agent_Helper._plan(me, planner_inputs)
    ah.Agent_Helper.reset(me)
    np.random.seed(cfg["seed"])
    rows, visited, collision = [], [], []
    for s in chain["steps"]:
        script["stg"], script["stop"] = s["stg"], bool(s["stop"])
        inputs = {'obstacle': np.zeros((m, m), np.float32), 'exp_pred': np.zeros((m, m), np.float32), 'goal': np.zeros((m, m)),
                  'pose_pred': np.array(list(s["pose"]) + s["lmb"], np.float64), 'found_goal': s["found"], 'goal_name': 'chair'}
        out = ah.Agent_Helper.plan_act(me, inputs)
        assert set(out) == {'action'} and out['action'] == me.last_action
        assert np.isin(me.visited_vis, (0, 1)).all() and np.isin(me.collision_map, (0, 1)).all()
        rows.append([out['action'], me.col_width, me.prev_blocked, me.forward_after_stop, me._previous_action, me.last_action,
                     me.untrap.total_id, me.untrap.epi_id, me.timestep, me.last_start[0], me.last_start[1],
                     int(me.collision_map.sum()), int(me.visited_vis.sum())])
        visited.append(me.visited_vis.astype(np.uint8))
        collision.append(me.collision_map.astype(np.uint8))
    return np.array(rows, np.int64), np.array(visited), np.array(collision)


def generate():
    ah, _ = load_reference()
    out = {}
    for name, chain in pc.chains().items():
        state, visited, collision = run_chain(ah, chain)
        assert state.shape == (len(chain["steps"]), len(pc.STATE))
        out[f"{name}/state"], out[f"{name}/visited"], out[f"{name}/collision"] = state, visited, collision
        pc.CLAIMS[name](chain, dict(state=state, visited=visited, collision=collision))
        print(f"[plan] {name:14s} {len(chain['steps']):3d} steps  actions {''.join(str(a) for a in state[:, 0])}  "
              f"collision cells {state[-1, 11]}  visited cells {state[-1, 12]}")
    np.savez_compressed(pc.GOLDEN, **out)
    print(f"[plan] -> {pc.GOLDEN} ({os.path.getsize(pc.GOLDEN)} bytes)")


if __name__ == "__main__":
    generate()
