"""Times the motion planner's step at the deployed size: a 480 x 480 local map in a 960 x 960 full map, col_rad 4, on the wall
maze of tools/bench_stg.py.

Rows, each with its sides alternated in one process, medians with [min, max] over ``--repeats`` windows of ``--calls`` calls:

* ``plan_mark``  the mark of a step of E = 1 / 4 / 8 / 16 episodes (a 26-point line and two collision cells each): one
                 ``peanut_plan_mark(_batch)`` launch against the only route there was before it -- the same writes as 26 slice
                 assignments and the index assignments in torch on the device maps, per episode.  Both sides are timed to the end
                 of the device work; the maps of the two sides are compared.
* ``plan_act``   ``Agent_Helper.plan_act`` per step (state machine, mark, short-term goal) against ``ShortTermGoal.get_stg`` alone
                 on the same maps, and against ``plan_act`` with the torch route for its mark.

    python -m tools.bench_plan [--out profiles/plan/plan.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_stg import maze                      # noqa: E402


def spread(v):
    v = sorted(v)
    return {"median": round(statistics.median(v), 4), "min": round(v[0], 4), "max": round(v[-1], 4), "n": len(v)}


def torch_mark(visited, collision, lmb, points, cells):
    """The route without the kernel: ``draw_line``'s 26 slice assignments on the window view, then the cells."""
    mat = visited[lmb[0]:lmb[1], lmb[2]:lmb[3]]
    for x, y in points:
        mat[x - 1:x + 1, y - 1:y + 1] = 1
    for r, c in cells:
        collision[r, c] = 1


def measure(sides, calls, repeats):
    for fn in sides.values():
        fn(3)
    t = {name: [] for name in sides}
    for _ in range(repeats):
        for name, fn in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(calls)
            torch.cuda.synchronize()
            t[name].append((time.perf_counter() - t0) / calls * 1e6)
    return {k: spread(v) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plan", "plan.jsonl"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_plan measures on the GPU; no device is visible")
    from peanut_amd import agent_helper as ah
    from peanut_amd.agent_state import default_args
    from peanut_amd.planner import ShortTermGoal
    dev = torch.device("cuda:0")
    args = default_args(goal_map=True, plan_stg=True, plan_act=True)
    m, full = 480, 960
    ob, lmb = maze(0)
    o = lmb[0]
    ob[o + 192:o + 209, o + 252:o + 269] = 0
    rows = []
    # ---- the mark alone ----
    for E in (1, 4, 8, 16):
        maps = {side: [(torch.zeros((full, full), dtype=torch.uint8, device=dev), torch.zeros((full, full), dtype=torch.uint8, device=dev))
                       for _ in range(E)] for side in ("torch", "kernel")}
        steps = [((200 + e, 260), (205 + e, 262 + e), [(o + 205 + e, o + 270), (o + 205 + e, o + 271)]) for e in range(E)]
        points = [[tuple(int(v) for v in p) for p in ah.plan_line(ls, st)] for ls, st, _ in steps]

        def by_torch(n, E=E, maps=maps, steps=steps, points=points):
            for _ in range(n):
                for e in range(E):
                    torch_mark(maps["torch"][e][0], maps["torch"][e][1], lmb, points[e], steps[e][2])

        def by_kernel(n, E=E, maps=maps, steps=steps):
            for _ in range(n):
                ah.plan_mark_batch([(maps["kernel"][e][0], maps["kernel"][e][1], lmb) + steps[e] for e in range(E)])
        sp = measure({"torch": by_torch, "kernel": by_kernel}, a.calls, a.repeats)
        same = all(torch.equal(maps["torch"][e][k], maps["kernel"][e][k]) for e in range(E) for k in range(2))
        rows.append({"bench": "plan_mark", "E": E, "us_per_step_of_E": sp, "torch_over_kernel": round(sp["torch"]["median"] / sp["kernel"]["median"], 2),
                     "maps_identical": bool(same), "cells_set": int(maps["kernel"][0][0].sum()) + int(maps["kernel"][0][1].sum()), "calls": a.calls})
    # ---- the whole step ----
    obstacle = torch.from_numpy(ob).to(dev)[lmb[0]:lmb[1], lmb[2]:lmb[3]]           # a view, as local_map[0] after update_full_map
    goal = torch.zeros((m, m), dtype=torch.uint8, device=dev)
    goal[430, 40] = 1
    # the agent steps to and fro between two places 0.25 m apart (no bump: the untrap's random turns would make the sides differ)
    cells = [(200.5, 260.25), (200.5, 265.25)]
    inputs = [{'obstacle': obstacle, 'goal': goal, 'pose_pred': np.array([(o + c) * 5 / 100.0, (o + r) * 5 / 100.0, 0.0] + lmb, np.float64),
               'found_goal': 0, 'goal_name': 'chair'} for r, c in cells]

    def helper():
        stg = ShortTermGoal(args, device=dev)
        st = SimpleNamespace(args=args, device=dev, stg=None, stg_stop=None, collision_map=torch.zeros((full, full), dtype=torch.uint8, device=dev),
                             visited_vis=torch.zeros((full, full), dtype=torch.uint8, device=dev), _stg_planner=lambda: stg,
                             next_preset_goal=lambda: None)
        h = ah.Agent_Helper(args, st)
        h.reset()
        return h
    h_kernel, h_torch, alone = helper(), helper(), helper()
    actions = {"kernel": [], "torch": []}

    def plan_act(n):
        for _ in range(n):
            actions["kernel"].append(h_kernel.plan_act(inputs[len(actions["kernel"]) % 2])['action'])

    def plan_act_torch(n):
        real = ah.plan_mark_batch
        ah.plan_mark_batch = lambda marks: [torch_mark(v, c, w, [tuple(int(q) for q in p) for p in ah.plan_line(ls, st)], cells)
                                            for v, c, w, ls, st, cells in marks]
        try:
            for _ in range(n):
                actions["torch"].append(h_torch.plan_act(inputs[len(actions["torch"]) % 2])['action'])
        finally:
            ah.plan_mark_batch = real

    def get_stg(n):
        st = alone.agent_states
        for k in range(n):
            st._stg_planner().get_stg(obstacle, goal, st.collision_map, st.visited_vis, lmb, list(cells[k % 2]), 0, 'chair')
    calls = max(1, a.calls // 4)
    sp = measure({"get_stg_alone": get_stg, "plan_act": plan_act, "plan_act_torch_marks": plan_act_torch}, calls, a.repeats)
    same = actions["kernel"] == actions["torch"] and all(
        torch.equal(getattr(h_kernel.agent_states, k), getattr(h_torch.agent_states, k)) for k in ("visited_vis", "collision_map"))
    rows.append({"bench": "plan_act", "local_map": m, "col_rad": int(args.col_rad), "us_per_step": sp,
                 "plan_act_minus_get_stg_us": round(sp["plan_act"]["median"] - sp["get_stg_alone"]["median"], 1),
                 "sides_identical": bool(same), "actions_seen": sorted(set(int(v) for v in actions["kernel"])),
                 "collision_cells": int(h_kernel.agent_states.collision_map.sum()), "calls": calls})
    for r in rows:
        r.update(device=torch.cuda.get_device_name(0), repeats=a.repeats)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main()
