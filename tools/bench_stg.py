"""Times the short-term goal at the deployed size: a 480 x 480 local map in a 960 x 960 full map, col_rad 4, on the wall mazes of
tools/bench_lockstep.py (the front crosses the whole map).

Sides, alternated in one process, medians with spread over ``--repeats`` windows of ``--calls`` calls each:

* ``get_stg``        ``ShortTermGoal.get_stg``, one solve: maps in, ``(stg, stop)`` out, one 24-byte read-back;
* ``host_window``    the route without this feature, with the two padded masks GIVEN on the device (nothing built them there
                     before): ``FMMPlanner.set_multi_goal`` + ``get_short_term_goal``, i.e. the same solve, then the copy of the
                     482 x 482 float64 field to the host, ``np.pad`` and the window arithmetic in NumPy;
* ``retry``          a start fenced in by a one-cell line: first solve, eroded map, second solve;
* ``magnify4``       a found goal farther than 100 cells with the step limit at four: five solves.

    python -m tools.bench_stg [--out profiles/stg/stg.jsonl]

``--batch`` (written to profiles/stg/stg_batch.jsonl): the same map on E DIFFERENT mazes (``maze(seed)``), E = 2, 4, 8 and 16:
E ``get_stg`` calls in a row against one ``get_stg_batch`` (``peanut_stg_plan_batch``), alternated in one process, milliseconds per
step of E episodes; and a mixed row at E = 8 -- six plain episodes, one ``retry``, one ``magnify4`` -- through the C ABI on both sides
(the step limit of four is not a planner argument).  ``earns_default``: the batch median lies below the singles' median by more than
the min-max spreads of both sides together.

    python -m tools.bench_stg --batch [--out profiles/stg/stg_batch.jsonl]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    v = sorted(v)
    return {"median": round(statistics.median(v), 4), "min": round(v[0], 4), "max": round(v[-1], 4), "n": len(v)}


def maze(seed, size=960, window=480):
    """tools/bench_lockstep.py: _maze_inputs, one episode; the local window in the middle, the agent's surroundings cleared."""
    rng = np.random.RandomState(100 + seed)
    ob = np.zeros((size, size), np.float32)
    for _ in range(int(0.012 * size * size / 20)):
        r, c, k = rng.randint(0, size), rng.randint(0, size), rng.randint(10, 60)
        if rng.rand() < 0.5:
            ob[r:r + 2, c:c + k] = 1
        else:
            ob[r:r + k, c:c + 2] = 1
    o = (size - window) // 2
    return ob, [o, o + window, o, o + window]


def batch_rows(a):
    """The ``--batch`` rows: one per E, then the mixed one."""
    from peanut_amd import _lib
    from peanut_amd.agent_state import default_args
    from peanut_amd.planner import ShortTermGoal, get_stg_batch
    import workspace_cases as wc
    dev = torch.device("cuda:0")
    args = default_args()
    m, full, emax = 480, 960, 16
    start = [200.5, 260.25]
    goal = torch.zeros((m, m), dtype=torch.uint8, device=dev)
    goal[430, 40] = 1
    col = torch.zeros((full, full), dtype=torch.uint8, device=dev)
    vis = torch.zeros((full, full), dtype=torch.uint8, device=dev)
    obstacles, lmb = [], None
    for e in range(emax):
        ob, lmb = maze(e)
        o = lmb[0]
        ob[o + 192:o + 209, o + 252:o + 269] = 0
        obstacles.append(torch.from_numpy(ob).to(dev)[lmb[0]:lmb[1], lmb[2]:lmb[3]])      # views, as local_map[0]
    fenced = obstacles[6].clone()                                                          # the retry episode of the mixed row
    fenced[192, 252:269] = fenced[208, 252:269] = 1
    fenced[192:209, 252] = fenced[192:209, 268] = 1
    planners = [ShortTermGoal(args, device=dev) for _ in range(emax)]
    lib = planners[0]._lib

    def measure(sides, calls):
        for fn in sides.values():
            fn(2)
        t = {name: [] for name in sides}
        for _ in range(a.repeats):
            for name, fn in sides.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(calls)
                torch.cuda.synchronize()
                t[name].append((time.perf_counter() - t0) / calls * 1e3)
        sp = {k: spread(v) for k, v in t.items()}
        gain = sp["singles"]["median"] - sp["batch"]["median"]
        noise = (sp["singles"]["max"] - sp["singles"]["min"]) + (sp["batch"]["max"] - sp["batch"]["min"])
        return sp, round(sp["singles"]["median"] / sp["batch"]["median"], 3), bool(gain > noise)
    rows = []
    calls = max(1, a.calls // 5)
    for E in (2, 4, 8, 16):
        ins = [(obstacles[e], goal, col, vis, lmb, start, 0, "chair") for e in range(E)]
        last = {}

        def singles(n, E=E, ins=ins, last=last):
            for _ in range(n):
                for e in range(E):
                    planners[e].get_stg(*ins[e])
            last["singles"] = [dict(planners[e].last) for e in range(E)]

        def batch(n, E=E, ins=ins, last=last):
            for _ in range(n):
                get_stg_batch(planners[:E], ins)
            last["batch"] = [dict(planners[e].last) for e in range(E)]
        sp, ratio, earns = measure({"singles": singles, "batch": batch}, calls)
        rows.append({"bench": "stg_batch", "E": E, "ms_per_step_of_E": sp, "singles_over_batch": ratio, "earns_default": earns,
                     "bit_identical": bool(wc.same(last["singles"], last["batch"])), "n_solves": [r["n_solves"] for r in last["batch"]],
                     "waves": planners[0].waves, "calls": calls})
    # the mixed row: six plain, one retry, one magnify4 (found goal, step limit four: five solves)
    E = 8
    obst = obstacles[:6] + [fenced, obstacles[7]]
    found, maxmag = [0] * 7 + [1], [8] * 7 + [4]
    res = (_lib.StgResultC * E)()
    ptr = lambda vals: (C.c_void_p * E)(*vals)                   # noqa: E731
    keep = dict(h=ptr([p._h.value for p in planners[:E]]), obstacle=ptr([o.data_ptr() for o in obst]),
                row_stride=(C.c_longlong * E)(*[int(o.stride(0)) for o in obst]), goal_map=ptr([goal.data_ptr()] * E),
                collision=ptr([col.data_ptr()] * E), visited=ptr([vis.data_ptr()] * E), lmb=(C.c_int * (4 * E))(*(list(lmb) * E)),
                start_exact=(C.c_double * (2 * E))(*(start * E)), found_goal=(C.c_int * E)(*found), radius_found=(C.c_int * E)(*[8] * E),
                magnify_when_hard=(C.c_double * E)(*[100.0] * E), max_magnify=(C.c_int * E)(*maxmag))
    desc = _lib.StgBatchC(size=C.sizeof(_lib.StgBatchC), E=E, reserved=0, result_out=res, stream=_lib.current_stream_ptr(dev), **keep)
    one = _lib.StgResultC()
    bounds, st = (C.c_int * 4)(*lmb), (C.c_double * 2)(*start)
    last = {}

    def fields(r):
        return [float(r.stg_x), float(r.stg_y), float(r.distance), int(r.stop), int(r.replan), int(r.retried), int(r.n_magnify), int(r.n_solves)]

    def singles(n):
        for _ in range(n):
            out = []
            for e in range(E):
                rc = lib.peanut_stg_plan(planners[e]._h, obst[e].data_ptr(), int(obst[e].stride(0)), goal.data_ptr(), col.data_ptr(), vis.data_ptr(),
                                         C.byref(bounds), C.byref(st), found[e], 8, 100.0, maxmag[e], C.byref(one), None, None, None,
                                         _lib.current_stream_ptr(dev))
                _lib.check(rc, "peanut_stg_plan")
                out.append(fields(one))
            last["singles"] = out

    def batch(n):
        for _ in range(n):
            _lib.check(lib.peanut_stg_plan_batch(C.byref(desc)), "peanut_stg_plan_batch")
        last["batch"] = [fields(res[e]) for e in range(E)]
    sp, ratio, earns = measure({"singles": singles, "batch": batch}, calls)
    rows.append({"bench": "stg_batch_mixed", "E": E, "episodes": "six plain, one retry, one magnify4", "ms_per_step_of_E": sp,
                 "singles_over_batch": ratio, "earns_default": earns, "bit_identical": last["singles"] == last["batch"],
                 "n_solves": [r[7] for r in last["batch"]], "waves": planners[0].waves, "calls": calls})
    for r in rows:
        r.update(device=torch.cuda.get_device_name(0), local_map=m, col_rad=int(args.col_rad), repeats=a.repeats)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", action="store_true", help="E single calls against one batched call -> profiles/stg/stg_batch.jsonl")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "stg", "stg_batch.jsonl" if a.batch else "stg.jsonl")
    if not torch.cuda.is_available():
        sys.exit("bench_stg measures on the GPU; no device is visible")
    if a.batch:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        rows = batch_rows(a)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")
                print(json.dumps(row))
        return
    from peanut_amd import _lib
    from peanut_amd.agent_state import default_args
    from peanut_amd.goal import FMMPlanner, GeodesicSolver
    from peanut_amd.planner import ShortTermGoal
    dev = torch.device("cuda:0")
    args = default_args()
    m, full = 480, 960
    ob, lmb = maze(0)
    start = [200.5, 260.25]
    o = lmb[0]
    ob[o + 192:o + 209, o + 252:o + 269] = 0
    full_ob = torch.from_numpy(ob).to(dev)
    obstacle = full_ob[lmb[0]:lmb[1], lmb[2]:lmb[3]]                    # a view, as local_map[0] after update_full_map
    fenced = obstacle.clone()                                           # the retry: a one-cell line around the start
    fenced[192, 252:269] = fenced[208, 252:269] = 1
    fenced[192:209, 252] = fenced[192:209, 268] = 1
    goal = torch.zeros((m, m), dtype=torch.uint8, device=dev)
    goal[430, 40] = 1
    col = torch.zeros((full, full), dtype=torch.uint8, device=dev)
    vis = torch.zeros((full, full), dtype=torch.uint8, device=dev)
    stg = ShortTermGoal(args, device=dev)
    stg.get_stg(obstacle, goal, col, vis, lmb, start, 0, "chair", taps=True)
    first = dict(stg.last)
    trav_dev, goal_dev = first["trav"].clone(), first["goal"].clone()
    solver = GeodesicSolver(m + 2, m + 2, 0, device=dev)
    state = [start[0] + 1, start[1] + 1]
    last = {}

    def get_stg(n):
        for _ in range(n):
            last["get_stg"] = stg.get_stg(obstacle, goal, col, vis, lmb, start, 0, "chair")

    def host_window(n):
        for _ in range(n):
            p = FMMPlanner(trav_dev, solver=solver)
            p.set_multi_goal(goal_dev)
            last["host_window"] = p.get_short_term_goal(state)

    def retry(n):
        for _ in range(n):
            stg.get_stg(fenced, goal, col, vis, lmb, start, 0, "chair")
            last["retry"] = dict(stg.last)

    res = _lib.StgResultC()

    def magnify4(n):
        bounds, st = (C.c_int * 4)(*lmb), (C.c_double * 2)(*start)
        for _ in range(n):
            rc = stg._lib.peanut_stg_plan(stg._h, obstacle.data_ptr(), int(obstacle.stride(0)), goal.data_ptr(), col.data_ptr(), vis.data_ptr(),
                                          C.byref(bounds), C.byref(st), 1, 8, 100.0, 4, C.byref(res), None, None, None,
                                          _lib.current_stream_ptr(dev))
            _lib.check(rc, "peanut_stg_plan")
        last["magnify4"] = dict(n_magnify=int(res.n_magnify), n_solves=int(res.n_solves), distance=float(res.distance))

    sides = [("get_stg", get_stg), ("host_window", host_window), ("retry", retry), ("magnify4", magnify4)]
    for _, fn in sides:
        fn(3)
    t = {name: [] for name, _ in sides}
    for _ in range(a.repeats):
        for name, fn in sides:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(a.calls)
            torch.cuda.synchronize()
            t[name].append((time.perf_counter() - t0) / a.calls * 1e3)
    hw = last["host_window"]
    same = (float(hw[0]) - 1, float(hw[1]) - 1) == last["get_stg"][0] and bool(hw[3]) == last["get_stg"][1] and \
        float(hw[2]) == first["distance"]
    row = {"bench": "stg", "device": torch.cuda.get_device_name(0), "local_map": m, "col_rad": int(args.col_rad), "calls": a.calls,
           "ms_per_call": {k: spread(v) for k, v in t.items()}, "one_solve": {"stg": first["stg"], "distance": first["distance"],
                                                                               "rounds": solver.rounds, "passes": solver.passes},
           "host_window_equals_get_stg": bool(same), "retry": {k: last["retry"][k] for k in ("retried", "n_solves", "distance")},
           "magnify4": last["magnify4"], "field_copy_bytes": (m + 2) * (m + 2) * 8,
           "get_stg_over_host_window": round(spread(t["get_stg"])["median"] / spread(t["host_window"])["median"], 3)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(row) + "\n")
    print(json.dumps(row))


if __name__ == "__main__":
    main()
