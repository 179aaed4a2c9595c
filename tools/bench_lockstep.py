#!/usr/bin/env python3
"""Several episodes per GPU in lock-step against the same episodes one after the other, for E = 1, 2, 4, 8, in ONE process,
the two sides alternating (A B A B A B: three repeats each, the spread of the three goes into the record):

  (a) stage 2 alone: E sequential `Agent_State.update_local_map` (forward + pose read-back + mark_agent each) against one
      `Agent_State_Group.update_local_maps` (forward_batch + ONE read-back + mark_agent_batch), microseconds per step of
      E episodes, wall clock between device synchronisations (both sides end every step on a read-back);
  (b) the config-4 pipeline shape of tools/configs_bench.py (Mask R-CNN R-101-FPN in the loop, 40-frame synthetic episodes
      of tools/bench_pipeline.py, 720 x 720 prediction + goal selection): E sequential `run_episode` calls against one
      `run_episodes`, steps/s/GPU summed over the episodes.

  (c) goal selection alone: E solvers on E different 960 x 960 maps (`goal`: the pipeline's synthetic episodes after 24 frames,
      whose agent stands inside an obstacle so that the field ends at once; `goal_mazes`: seeded wall mazes the front crosses): E
      `GeodesicSolver.select` calls against one `goal.select_batch`, with and without the preceding begin, milliseconds per
      step of E episodes, wall clock around calls that end in their own synchronise; and the pipeline of (b) with
      `batch_goals` off as a third column.  In a tree whose package has no `select_batch` (an older commit, for a side-by-side
      run of its library) the sequential sides alone are measured.

  (d) the goal map of the planner inputs (`goalmap`, --goalmap-only, written to <out>/goalmap.jsonl): on E 480 x 480 local maps with
      blobs of the goal category and of others, E `peanut_goal_map` calls against one `peanut_goal_map_batch` (device events around a
      chain of calls, microseconds per step of E episodes), `Agent_State.update_goal_map` E times against one
      `Agent_State_Group.update_goal_maps` with their read-backs (wall clock), the reference's statements on the same machine as the
      host baseline (torch sum, `.cpu()`, the scipy chain scikit-image calls; milliseconds per episode), and the lock-step pipeline
      of (b) with `args.goal_map` off and on.

  (e) the short-term goals in the pipeline (`stg_pipeline`, --plan-stg, written to <out>/plan_stg.jsonl): the pipeline of (b) with
      `args.goal_map` and `args.plan_stg` on at E = 4 and 8, `Agent_State_Group.short_term_goals` after every step with `batch_stg`
      off (E `peanut_stg_plan` in a row) and on (one `peanut_stg_plan_batch`), and the same pipeline without the call.

  (g) the motor action in the pipeline (`plan_act_pipeline`, --plan-act, written to profiles/plan/lockstep_plan_act.jsonl): the pipeline
      of (e) with `batch_stg` on, the motor action off (`short_term_goals` after every step) and on (`plan_acts`: one
      `peanut_plan_mark_batch`, the same batched short-term goals, the host state machines), alternating on one set of states.

  (f) recording map sequences in the pipeline (`record_maps`, --record-maps, written to profiles/mapio/recorder.jsonl): the lock-step
      pipeline of (b) with 100-frame episodes (save steps 25, 50, 75, 100 of nav/collect_maps.py:52) without a recorder, with a host
      recorder built from the route of `mapio.encode_map` (the fp32 full map copied down, two NumPy passes,
      E times in a row) and with `mapio.MapSequenceRecorder` (one launch per save step, nothing read back during the episode).

    python tools/bench_lockstep.py [--out profiles/lockstep] [--no-pipeline] [--no-trace] [--goal-only] [--pipeline-only] [--goalmap-only]
                                   [--plan-stg] [--plan-act] [--record-maps]

writes <out>/lockstep.json.  Kernel counts and idle gaps per stage-2 step come from one `rocprofv3 --kernel-trace --stats` run
of this file's `--trace-child` mode (no counters in that run), summarised under "trace" in the same record."""
import argparse
import glob
import json
import os
import sqlite3
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

BATCHES = (1, 2, 4, 8)
GOAL_BATCHES = (1, 2, 4, 8, 16)


def _stage2_obs(E, dev, seed=0):
    """E observations [E,14,120,160]: a slanted wall 1.5-4 m away with sensor noise, three semantic rectangles."""
    g = torch.Generator().manual_seed(seed)
    obs = torch.zeros(E, 14, 120, 160)
    for e in range(E):
        wall = 150.0 + 250.0 * torch.rand(1, generator=g).item()
        cols = torch.arange(160.0)[None, :] - 80.0
        obs[e, 3] = (wall + 0.4 * cols).clamp(50.0, 495.0) + torch.rand((120, 160), generator=g)
        for k in (1, 4, 6):
            r0, c0 = int(torch.randint(10, 80, (1,), generator=g)), int(torch.randint(5, 120, (1,), generator=g))
            obs[e, 4 + k, r0:r0 + 30, c0:c0 + 30] = 1.0
    return obs.to(dev)


def _spread(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 3), "min": round(v[0], 3), "max": round(v[-1], 3), "runs": [round(x, 3) for x in v]}


def _stage2_sides(E, dev):
    from peanut_amd.agent_state import Agent_State, Agent_State_Group, default_args
    args = default_args(sem_gpu_id=dev.index)
    seq = [Agent_State(args, prediction_model=None) for _ in range(E)]
    lock = [Agent_State(args, prediction_model=None) for _ in range(E)]
    for s in seq + lock:
        s.reset()
    grp = Agent_State_Group(lock)
    obs = _stage2_obs(E, dev)
    pose = [0.0, 0.0, 0.05]                                   # the agent turns on the spot: it stays inside its local map
    each = [obs[e:e + 1] for e in range(E)]

    def sequential(n):
        for _ in range(n):
            for s, o in zip(seq, each):
                s.poses = s._upload_pose(pose)
                s.update_local_map(o)

    def batched(n):
        for _ in range(n):
            grp.update_local_maps(obs, [pose] * E)
    return sequential, batched, (seq, lock, grp)


def stage2(dev, steps=2000, repeats=3):
    out = {}
    for E in BATCHES:
        sequential, batched, keep = _stage2_sides(E, dev)
        sequential(20)
        batched(20)
        t = {"sequential": [], "batched": []}
        for _ in range(repeats):
            for name, fn in (("sequential", sequential), ("batched", batched)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(steps)
                torch.cuda.synchronize()
                t[name].append((time.perf_counter() - t0) / steps * 1e6)
        seq, lock, _ = keep
        same = all(torch.equal(a.local_map, b.local_map) and torch.equal(a.local_pose, b.local_pose) for a, b in zip(seq, lock))
        out[str(E)] = {"sequential_us_per_step": _spread(t["sequential"]), "batched_us_per_step": _spread(t["batched"]),
                       "speedup_median": round(_spread(t["sequential"])["median"] / _spread(t["batched"])["median"], 3),
                       "maps_and_poses_bit_identical": bool(same)}
        print(f"stage 2, E = {E}: {out[str(E)]}", file=sys.stderr, flush=True)
        del keep
    return out


def forward_only(dev, steps=2000, repeats=3):
    """`Semantic_Mapping.forward` alone (the figure README "Measured" records for the map projection step: device events around a
    chain of steps, no read-back) and `forward_batch` alone at every E, alternating, microseconds per call."""
    from peanut_amd.agent_state import default_args
    from peanut_amd.mapping import Semantic_Mapping
    args = default_args(sem_gpu_id=dev.index)
    args.device = dev
    sm = Semantic_Mapping(args)
    sm.reserve(max(BATCHES))
    M = sm.map_cells
    obs = _stage2_obs(max(BATCHES), dev)
    rel = torch.tensor([0.0, 0.0, 0.05], device=dev).repeat(max(BATCHES), 1).contiguous()
    out = {}
    for E in BATCHES:
        bufs = [[torch.zeros(14, M, M, device=dev) for _ in range(E)] for _ in range(2)]
        fp1, fpE = torch.empty(1, 100, 100, device=dev), torch.empty(E, 100, 100, device=dev)
        poses = torch.tensor([12.0, 12.0, 0.0], device=dev).repeat(E, 1).contiguous()

        def single(n):
            for i in range(n):
                a, b = bufs[i & 1], bufs[1 - (i & 1)]
                for e in range(E):
                    sm(obs[e:e + 1], rel[e], a[e], poses[e], None, out=(fp1, b[e]))

        def batch(n):
            for i in range(n):
                sm.forward_batch(obs[:E], rel[:E], bufs[i & 1], poses, out=(fpE, bufs[1 - (i & 1)]))
        single(20)
        batch(20)
        t = {"single": [], "batch": []}
        for _ in range(repeats):
            for name, fn in (("single", single), ("batch", batch)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                fn(steps)
                e1.record()
                torch.cuda.synchronize()
                t[name].append(e0.elapsed_time(e1) / steps * 1e3)
        out[str(E)] = {"E_single_forwards_us": _spread(t["single"]), "one_forward_batch_us": _spread(t["batch"])}
        print(f"forward only, E = {E}: {out[str(E)]}", file=sys.stderr, flush=True)
    return out


def pipeline(dev, frames=40, repeats=3, batches=BATCHES):
    import gc
    import inspect

    from bench_pipeline import synth_episode
    from peanut_amd.agent_state import Agent_State, default_args
    from peanut_amd.prediction import PEANUT_Prediction_Model
    from peanut_amd.rcnn_weights import RcnnCfg, make_seeded_rcnn_state_dict
    from peanut_amd.replay import run_episode, run_episodes
    from peanut_amd.segmentation import HipDetector
    from peanut_amd.weights import PredCfg, make_seeded_state_dict
    args = default_args(only_explore=0, sem_gpu_id=dev.index, pred_precision="fp32", select_goal=True)
    model = PEANUT_Prediction_Model(args, state_dict=make_seeded_state_dict(PredCfg(), 0))
    rcfg = RcnnCfg(score_thresh_test=0.5)
    det = HipDetector(rcfg, make_seeded_rcnn_state_dict(rcfg, 0), device=dev)
    emax = max(batches)
    eps = [synth_episode(1000 + e, frames, dev) for e in range(emax)]
    for ep in eps:
        for fr in ep:
            for k in ("masks", "classes", "scores"):
                fr.pop(k)
    seq = [Agent_State(args, prediction_model=model) for _ in range(emax)]
    lock = [Agent_State(args, prediction_model=model) for _ in range(emax)]
    out = {}
    for E in batches:
        goals = [3] * E

        def sequential():
            return sum(run_episode(seq[e], eps[e], goal_cat=3, detector=det) for e in range(E))

        def lockstep():
            return sum(run_episodes(lock[:E], eps[:E], goals, detector=det))

        def lockstep_single_goals():
            return sum(run_episodes(lock[:E], eps[:E], goals, detector=det, batch_goals=False))
        sides = [("sequential", sequential), ("lockstep", lockstep)]
        if "batch_goals" in inspect.signature(run_episodes).parameters:
            sides.append(("lockstep_single_goals", lockstep_single_goals))
        run_episode(seq[0], eps[0][:12], goal_cat=3, detector=det)            # warm-up: plans and workspaces of both batch sizes
        run_episodes(lock[:E], [ep[:12] for ep in eps[:E]], goals, detector=det)
        gc.collect()
        t = {name: [] for name, _ in sides}
        preds = {}
        for _ in range(repeats):
            for name, fn in sides:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                preds[name] = fn()
                torch.cuda.synchronize()
                t[name].append(E * frames / (time.perf_counter() - t0))
        out[str(E)] = {"sequential_steps_per_s": _spread(t["sequential"]), "lockstep_steps_per_s": _spread(t["lockstep"]),
                       "speedup_median": round(_spread(t["lockstep"])["median"] / _spread(t["sequential"])["median"], 3),
                       "predictions": preds}
        if "lockstep_single_goals" in t:
            out[str(E)]["lockstep_single_goals_steps_per_s"] = _spread(t["lockstep_single_goals"])
        print(f"pipeline, E = {E}: {out[str(E)]}", file=sys.stderr, flush=True)
    return out


GOALMAP_BATCHES = (1, 4, 8, 16)


def _goalmap_maps(dev, n, m=480, seed=7):
    """n local maps [14, m, m]: per map a few blobs of the goal category (channel 4 + e % 6; every second map holds one large
    enough to survive three erosions), blobs of other categories over and beside them, values in [2^-10, 1]."""
    import numpy as np
    rng = np.random.RandomState(seed)
    maps, cns = [], []
    for e in range(n):
        lm = np.zeros((14, m, m), np.float32)
        cn = 4 + e % 6
        def blob(ch, lo, hi):
            h, w = rng.randint(lo, hi + 1, size=2)
            r0, c0 = rng.randint(0, m - h), rng.randint(0, m - w)
            lm[ch, r0:r0 + h, c0:c0 + w] = rng.uniform(2.0 ** -10, 1.0, size=(h, w))
        for _ in range(6):
            blob(cn, 1, 6)
        if e % 2 == 0:
            for _ in range(3):
                blob(cn, 12, 60)
        for _ in range(8):
            blob(4 + rng.randint(0, 10), 5, 60)
        maps.append(torch.from_numpy(lm).to(dev))
        cns.append(cn)
    return maps, cns


def _goalmap_host(lm, cn, n_erode=3):
    """The reference's statements (agent_state.py:430-446) on a device map: reduction, copy to the host, the scipy chain."""
    from scipy import ndimage as ndi
    if lm[cn].sum() != 0.:
        temp_goal = lm[cn].cpu().numpy() > 0
        for _ in range(n_erode):
            temp_goal = ndi.binary_erosion(temp_goal, border_value=1)
        temp_goal = ndi.binary_dilation(temp_goal).astype(float)
        temp_goal *= (torch.sum(lm[4:10], dim=0) - lm[cn]).cpu().numpy() == 0
        return int(temp_goal.sum() != 0.)
    return 0


def goalmap(dev, calls=500, repeats=3):
    import ctypes as C
    from types import SimpleNamespace

    from peanut_amd import _lib
    from peanut_amd.agent_state import Agent_State, Agent_State_Group, default_args
    lib = _lib.load()
    m = 480
    maps, cns = _goalmap_maps(dev, max(GOALMAP_BATCHES), m)
    outs = [torch.zeros((m, m), dtype=torch.uint8, device=dev) for _ in maps]
    found1 = torch.zeros(max(GOALMAP_BATCHES), dtype=torch.int32, device=dev)
    foundE = torch.zeros(max(GOALMAP_BATCHES), dtype=torch.int32, device=dev)
    stream = _lib.current_stream_ptr(dev)
    args = default_args(sem_gpu_id=dev.index, only_explore=0, goal_map=True)
    states = [Agent_State(args, prediction_model=SimpleNamespace()) for _ in maps]
    for s, lm, cn in zip(states, maps, cns):
        s.local_map, s.goal_cat, s.global_goals = lm, cn - 4, [[48, 48]]
    infos = [{"goal_name": "chair"}] * len(states)
    recs = []
    for E in GOALMAP_BATCHES:
        ptrs = (C.c_void_p * E)(*[t.data_ptr() for t in maps[:E]])
        ps, rs = (C.c_longlong * E)(*[m * m] * E), (C.c_longlong * E)(*[m] * E)
        pr = (C.c_int * (6 * E))(*[v for cn in cns[:E] for v in (cn, 1, 3, 1, 48, 48)])
        op = (C.c_void_p * E)(*[t.data_ptr() for t in outs[:E]])
        grp = Agent_State_Group(states[:E])

        def single(n):
            for _ in range(n):
                for e in range(E):
                    lib.peanut_goal_map(maps[e].data_ptr(), 14, m, m * m, m, cns[e], 1, 3, 1, 48, 48, outs[e].data_ptr(),
                                        found1.data_ptr() + 4 * e, stream)

        def batch(n):
            for _ in range(n):
                lib.peanut_goal_map_batch(E, ptrs, 14, m, ps, rs, pr, op, foundE.data_ptr(), stream)

        def single_state(n):
            for _ in range(n):
                for s, i in zip(states[:E], infos):
                    s.update_goal_map(i)

        def batch_state(n):
            for _ in range(n):
                grp.update_goal_maps(states[:E], infos[:E])
        single(3)
        ref_maps = [o.clone() for o in outs[:E]]
        batch(3)
        torch.cuda.synchronize()
        same = all(torch.equal(a, b) for a, b in zip(ref_maps, outs[:E])) and torch.equal(found1[:E], foundE[:E])
        t = {"single": [], "batch": [], "single_state": [], "batch_state": []}
        for _ in range(repeats):
            for name, fn in (("single", single), ("batch", batch)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                fn(calls)
                e1.record()
                torch.cuda.synchronize()
                t[name].append(e0.elapsed_time(e1) / calls * 1e3)
            for name, fn in (("single_state", single_state), ("batch_state", batch_state)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(calls)
                torch.cuda.synchronize()
                t[name].append((time.perf_counter() - t0) / calls * 1e6)
        host = []
        host_found = [_goalmap_host(maps[e], cns[e]) for e in range(E)]
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for e in range(E):
                _goalmap_host(maps[e], cns[e])
            host.append((time.perf_counter() - t0) * 1e3)
        rec = {"section": "goalmap", "E": E, "m": m, "E_single_calls_us": _spread(t["single"]), "one_batched_call_us": _spread(t["batch"]),
               "E_update_goal_map_us": _spread(t["single_state"]), "one_update_goal_maps_us": _spread(t["batch_state"]),
               "host_reference_statements_ms": _spread(host), "found": foundE[:E].cpu().tolist(),
               "batch_bits_equal_single": bool(same), "found_equals_host": foundE[:E].cpu().tolist() == host_found}
        print(f"goalmap, E = {E}: {rec}", file=sys.stderr, flush=True)
        recs.append(rec)
    return recs


def goalmap_pipeline(dev, frames=40, repeats=3, batches=(1, 4, 8)):
    """The lock-step pipeline of `pipeline` with `args.goal_map` off and on, alternating, on ONE set of states (the switch is
    flipped on their shared args: two sets of states differ by a percent or two through where their maps lie in memory)."""
    import gc

    from bench_pipeline import synth_episode
    from peanut_amd.agent_state import Agent_State, default_args
    from peanut_amd.prediction import PEANUT_Prediction_Model
    from peanut_amd.rcnn_weights import RcnnCfg, make_seeded_rcnn_state_dict
    from peanut_amd.replay import run_episodes
    from peanut_amd.segmentation import HipDetector
    from peanut_amd.weights import PredCfg, make_seeded_state_dict
    args = default_args(only_explore=0, sem_gpu_id=dev.index, pred_precision="fp32", select_goal=True, goal_map=False)
    both = {"off": False, "on": True}
    model = PEANUT_Prediction_Model(args, state_dict=make_seeded_state_dict(PredCfg(), 0))
    rcfg = RcnnCfg(score_thresh_test=0.5)
    det = HipDetector(rcfg, make_seeded_rcnn_state_dict(rcfg, 0), device=dev)
    emax = max(batches)
    eps = [synth_episode(1000 + e, frames, dev) for e in range(emax)]
    for ep in eps:
        for fr in ep:
            for k in ("masks", "classes", "scores"):
                fr.pop(k)
    states = [Agent_State(args, prediction_model=model) for _ in range(emax)]
    recs = []
    for E in batches:
        goals = [3] * E
        for name in both:
            args.goal_map = both[name]
            run_episodes(states[:E], [ep[:12] for ep in eps[:E]], goals, detector=det)
        gc.collect()
        t = {name: [] for name in both}
        maps, found = {}, []
        for _ in range(repeats):
            for name in both:
                args.goal_map = both[name]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run_episodes(states[:E], eps[:E], goals, detector=det)
                torch.cuda.synchronize()
                t[name].append(E * frames / (time.perf_counter() - t0))
                maps[name] = [s.full_map.clone() for s in states[:E]]
                found = [int(s.found_goal) for s in states[:E]]
        same = all(torch.equal(a, b) for a, b in zip(maps["off"], maps["on"]))
        rec = {"section": "goalmap_pipeline", "E": E, "frames": frames, "goal_map_off_steps_per_s": _spread(t["off"]),
               "goal_map_on_steps_per_s": _spread(t["on"]), "found_goal_last_step": found,
               "maps_bit_identical": bool(same)}
        print(f"goalmap pipeline, E = {E}: {rec}", file=sys.stderr, flush=True)
        recs.append(rec)
    return recs


def stg_pipeline(dev, frames=40, repeats=3, batches=(4, 8)):
    """The lock-step pipeline of `pipeline` with `args.goal_map` and `args.plan_stg` on and the group's `short_term_goals` after every
    step: `batch_stg` off (E `peanut_stg_plan` in a row) against on (one `peanut_stg_plan_batch`), alternating on ONE set of states,
    and the same pipeline without the call as the base line."""
    import gc

    from bench_pipeline import synth_episode
    from peanut_amd.agent_state import Agent_State, default_args
    from peanut_amd.peanut_agent import coco_goal_names
    from peanut_amd.prediction import PEANUT_Prediction_Model
    from peanut_amd.rcnn_weights import RcnnCfg, make_seeded_rcnn_state_dict
    from peanut_amd.replay import run_episodes
    from peanut_amd.segmentation import HipDetector
    from peanut_amd.weights import PredCfg, make_seeded_state_dict
    args = default_args(only_explore=0, sem_gpu_id=dev.index, pred_precision="fp32", select_goal=True, goal_map=True, plan_stg=True)
    model = PEANUT_Prediction_Model(args, state_dict=make_seeded_state_dict(PredCfg(), 0))
    rcfg = RcnnCfg(score_thresh_test=0.5)
    det = HipDetector(rcfg, make_seeded_rcnn_state_dict(rcfg, 0), device=dev)
    emax = max(batches)
    eps = [synth_episode(1000 + e, frames, dev) for e in range(emax)]
    for ep in eps:
        for fr in ep:
            for k in ("masks", "classes", "scores"):
                fr.pop(k)
    states = [Agent_State(args, prediction_model=model) for _ in range(emax)]
    name3 = coco_goal_names.get(3, "")
    sides = {"no_stg": None, "single": False, "batch": True}
    recs = []
    for E in batches:
        goals = [3] * E
        seen = {}

        def run(side, episodes):
            holder, out, solves = [], [], []

            def on_step(i, act, predicted):
                out.append(holder[0].short_term_goals([{"goal_name": name3}] * len(act)))
                solves.append([s._stg.last["n_solves"] for s in act])
            if sides[side] is None:
                run_episodes(states[:E], episodes, goals, detector=det)
            else:
                run_episodes(states[:E], episodes, goals, detector=det, on_step=on_step, on_group=holder.append, batch_stg=sides[side])
                seen[side] = (out, solves, holder[0].stg_batches)
        for side in sides:
            run(side, [ep[:12] for ep in eps[:E]])
        gc.collect()
        t = {side: [] for side in sides}
        for _ in range(repeats):
            for side in sides:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(side, eps[:E])
                torch.cuda.synchronize()
                t[side].append(E * frames / (time.perf_counter() - t0))
        solves = [n for step in seen["batch"][1] for n in step]
        ms = {side: 1e3 * E / _spread(t[side])["median"] for side in sides}      # per lock-step step of E episodes
        rec = {"section": "stg_pipeline", "E": E, "frames": frames, "no_stg_steps_per_s": _spread(t["no_stg"]),
               "batch_stg_off_steps_per_s": _spread(t["single"]), "batch_stg_on_steps_per_s": _spread(t["batch"]),
               "ms_per_lockstep_step": {k: round(v, 3) for k, v in ms.items()},
               "stg_adds_ms_per_step": {"single": round(ms["single"] - ms["no_stg"], 3), "batch": round(ms["batch"] - ms["no_stg"], 3)},
               "stg_batches": [seen["single"][2], seen["batch"][2]], "solves_per_episode_step": {"mean": round(sum(solves) / len(solves), 3), "max": max(solves)},
               "goals_identical": seen["single"][0] == seen["batch"][0]}
        print(f"stg pipeline, E = {E}: {rec}", file=sys.stderr, flush=True)
        recs.append(rec)
    return recs


def plan_act_pipeline(dev, frames=40, repeats=3, batches=(4, 8)):
    """The lock-step pipeline of `stg_pipeline` (config 4: detector, projection, prediction, goal selection, goal map, batched short-term
    goals) with the motor action switched off and on, alternating on ONE set of states: off = `short_term_goals` after every step, the
    `batch` side of `stg_pipeline`; on = `plan_acts` after every step (one `peanut_plan_mark_batch`, the same batched short-term goals,
    the host state machines).  The recorded frames do not follow the actions, so most forward actions meet a pose that moved as the
    recording says.  `off` is also held against the spread recorded for it in <out>/plan_stg.jsonl (reported, not asserted)."""
    import gc

    import numpy as np
    from bench_pipeline import synth_episode
    from peanut_amd.agent_helper import Agent_Helper
    from peanut_amd.agent_state import Agent_State, default_args
    from peanut_amd.peanut_agent import coco_goal_names
    from peanut_amd.prediction import PEANUT_Prediction_Model
    from peanut_amd.rcnn_weights import RcnnCfg, make_seeded_rcnn_state_dict
    from peanut_amd.replay import run_episodes
    from peanut_amd.segmentation import HipDetector
    from peanut_amd.weights import PredCfg, make_seeded_state_dict
    args = default_args(only_explore=0, sem_gpu_id=dev.index, pred_precision="fp32", select_goal=True, goal_map=True, plan_stg=True, plan_act=True)
    model = PEANUT_Prediction_Model(args, state_dict=make_seeded_state_dict(PredCfg(), 0))
    rcfg = RcnnCfg(score_thresh_test=0.5)
    det = HipDetector(rcfg, make_seeded_rcnn_state_dict(rcfg, 0), device=dev)
    emax = max(batches)
    eps = [synth_episode(1000 + e, frames, dev) for e in range(emax)]
    for ep in eps:
        for fr in ep:
            for k in ("masks", "classes", "scores"):
                fr.pop(k)
    states = [Agent_State(args, prediction_model=model) for _ in range(emax)]
    helpers = [Agent_Helper(args, s) for s in states]
    name3 = coco_goal_names.get(3, "")
    parent = {}
    try:
        with open(os.path.join(ROOT, "profiles", "lockstep", "plan_stg.jsonl")) as f:
            for line in f:
                r = json.loads(line)
                parent[r["E"]] = r["batch_stg_on_steps_per_s"]
    except OSError:
        pass
    recs = []
    for E in batches:
        goals = [3] * E
        seen = {}

        def run(side, episodes):
            holder, out = [], []

            def on_step(i, act, predicted):
                infos = [{"goal_name": name3}] * len(act)
                if side == "on":
                    out.append([a["action"] for a in holder[0].plan_acts(infos)])
                else:
                    out.append(holder[0].short_term_goals(infos))
            for h in helpers[:E]:
                h.reset()
            np.random.seed(0)
            run_episodes(states[:E], episodes, goals, detector=det, on_step=on_step, on_group=holder.append)
            seen[side] = out
        for side in ("off", "on"):
            run(side, [ep[:12] for ep in eps[:E]])
        gc.collect()
        t = {"off": [], "on": []}
        for _ in range(repeats):
            for side in t:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(side, eps[:E])
                torch.cuda.synchronize()
                t[side].append(E * frames / (time.perf_counter() - t0))
        ms = {side: 1e3 * E / _spread(t[side])["median"] for side in t}             # per lock-step step of E episodes
        actions = [a for step in seen["on"] for a in step]
        rec = {"section": "plan_act_pipeline", "E": E, "frames": frames, "plan_act_off_steps_per_s": _spread(t["off"]),
               "plan_act_on_steps_per_s": _spread(t["on"]), "ms_per_lockstep_step": {k: round(v, 3) for k, v in ms.items()},
               "plan_act_adds_ms_per_step": round(ms["on"] - ms["off"], 3), "actions": {str(a): actions.count(a) for a in sorted(set(actions))},
               "collision_cells": [int(s.collision_map.sum()) for s in states[:E]], "visited_cells": [int(s.visited_vis.sum()) for s in states[:E]]}
        if E in parent:
            med = _spread(t["off"])["median"]
            rec["parent_off_steps_per_s"] = parent[E]
            rec["off_inside_parent_spread"] = bool(parent[E]["min"] <= med <= parent[E]["max"])
        print(f"plan_act pipeline, E = {E}: {rec}", file=sys.stderr, flush=True)
        recs.append(rec)
    return recs


def visualize_pipeline(dev, frames=40, repeats=3, batches=(1, 4, 8)):
    """The lock-step pipeline of `plan_act_pipeline` (config 4, `plan_acts` after every step) with the visualisation frame, three
    sides alternating on ONE set of states: `off` = args.visualize 0 (the `on` side of `plan_act_pipeline`; held against the spread
    recorded for it in profiles/plan/lockstep_plan_act.jsonl -- reported, not asserted); `device` = args.visualize 1 (one
    `render_batch` and one pinned read-back per lock-step step, nothing written to disk); `host` = args.visualize 0 and, after every
    step, the reference's host statements (tools/bench_vis.host_frame: the plane downloads, NumPy, PIL, matplotlib, scipy) once per
    episode."""
    import gc

    import numpy as np
    from bench_pipeline import synth_episode
    from bench_vis import host_frame, host_tables
    from peanut_amd import vis as pv
    from peanut_amd.agent_helper import Agent_Helper
    from peanut_amd.agent_state import Agent_State, default_args
    from peanut_amd.peanut_agent import coco_goal_names
    from peanut_amd.prediction import PEANUT_Prediction_Model
    from peanut_amd.rcnn_weights import RcnnCfg, make_seeded_rcnn_state_dict
    from peanut_amd.replay import run_episodes
    from peanut_amd.segmentation import HipDetector
    from peanut_amd.weights import PredCfg, make_seeded_state_dict
    args = default_args(only_explore=0, sem_gpu_id=dev.index, pred_precision="fp32", select_goal=True, goal_map=True, plan_stg=True, plan_act=True)
    model = PEANUT_Prediction_Model(args, state_dict=make_seeded_state_dict(PredCfg(), 0))
    rcfg = RcnnCfg(score_thresh_test=0.5)
    det = HipDetector(rcfg, make_seeded_rcnn_state_dict(rcfg, 0), device=dev)
    emax = max(batches)
    eps = [synth_episode(1000 + e, frames, dev) for e in range(emax)]
    for ep in eps:
        for fr in ep:
            for k in ("masks", "classes", "scores"):
                fr.pop(k)
    states = [Agent_State(args, prediction_model=model) for _ in range(emax)]
    helpers = [Agent_Helper(args, s) for s in states]
    g = torch.Generator().manual_seed(1)
    for h in helpers:
        h.rgb_vis = (torch.rand((480, 640, 3), generator=g) * 256).to(torch.uint8).to(dev)
    name3 = coco_goal_names.get(3, "")
    palette, cm, disk4 = host_tables()
    background = pv.init_vis_image(name3, None)
    parent = {}
    try:
        with open(os.path.join(ROOT, "profiles", "plan", "lockstep_plan_act.jsonl")) as f:
            for line in f:
                r = json.loads(line)
                parent[r["E"]] = r["plan_act_on_steps_per_s"]
    except OSError:
        pass
    recs = []
    for E in batches:
        goals = [3] * E
        seen = {}

        def run(side, episodes):
            holder, out = [], []
            args.visualize = 1 if side == "device" else 0

            def on_step(i, act, predicted):
                infos = [{"goal_name": name3}] * len(act)
                out.append([a["action"] for a in holder[0].plan_acts(infos)])
                if side == "host":
                    for s in act:
                        p = s.planner_inputs(infos[0], host=False)
                        it = s.vis_item(p, stg=s.helper.stg, rgb=s.helper.rgb_vis)
                        if it["value"] is None:         # (visualize was off on this side: the solver's fields are fetched here)
                            it["dd_wt"], it["value"] = (None, None) if s.target_pred is None else s._goal_solver().fields()
                        s.helper.vis_image = host_frame(it, background, palette, args.num_sem_categories, cm, disk4)
            for h in helpers[:E]:
                h.reset()
            np.random.seed(0)
            run_episodes(states[:E], episodes, goals, detector=det, on_step=on_step, on_group=holder.append)
            seen[side] = out
        for side in ("off", "device", "host"):
            run(side, [ep[:12] for ep in eps[:E]])
        gc.collect()
        t = {"off": [], "device": [], "host": []}
        for _ in range(repeats):
            for side in t:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(side, eps[:E])
                torch.cuda.synchronize()
                t[side].append(E * frames / (time.perf_counter() - t0))
        args.visualize = 0
        assert seen["off"] == seen["device"] == seen["host"], "the frame changed an action"
        ms = {side: 1e3 * E / _spread(t[side])["median"] for side in t}             # per lock-step step of E episodes
        rec = {"section": "visualize_pipeline", "E": E, "frames": frames, **{f"visualize_{k}_steps_per_s": _spread(v) for k, v in t.items()},
               "ms_per_lockstep_step": {k: round(v, 3) for k, v in ms.items()},
               "device_adds_ms_per_step": round(ms["device"] - ms["off"], 3), "host_adds_ms_per_step": round(ms["host"] - ms["off"], 3)}
        if E in parent:
            med = _spread(t["off"])["median"]
            rec["parent_off_steps_per_s"] = parent[E]
            rec["off_inside_parent_spread"] = bool(parent[E]["min"] <= med <= parent[E]["max"])
        print(f"visualize pipeline, E = {E}: {rec}", file=sys.stderr, flush=True)
        recs.append(rec)
    return recs


def record_maps(dev, frames=100, repeats=3, batches=(4, 8)):
    """The lock-step pipeline of `pipeline` with no recorder, a host recorder (the fp32 map copied down and encoded with NumPy, per
    episode) and `mapio.MapSequenceRecorder`, alternating on ONE set of states; steps/s/GPU summed over the episodes.  After the
    timed runs the two recorders' sequences and keep decisions are compared."""
    import gc

    import numpy as np
    from bench_pipeline import synth_episode
    from peanut_amd import mapio
    from peanut_amd.agent_state import Agent_State, default_args
    from peanut_amd.prediction import PEANUT_Prediction_Model
    from peanut_amd.rcnn_weights import RcnnCfg, make_seeded_rcnn_state_dict
    from peanut_amd.replay import run_episodes
    from peanut_amd.segmentation import HipDetector
    from peanut_amd.weights import PredCfg, make_seeded_state_dict
    args = default_args(only_explore=0, sem_gpu_id=dev.index, pred_precision="fp32", select_goal=True)
    model = PEANUT_Prediction_Model(args, state_dict=make_seeded_state_dict(PredCfg(), 0))
    rcfg = RcnnCfg(score_thresh_test=0.5)
    det = HipDetector(rcfg, make_seeded_rcnn_state_dict(rcfg, 0), device=dev)
    emax = max(batches)
    eps = [synth_episode(1000 + e, frames, dev) for e in range(emax)]
    for ep in eps:
        for fr in ep:
            for k in ("masks", "classes", "scores"):
                fr.pop(k)
    states = [Agent_State(args, prediction_model=model) for _ in range(emax)]
    steps = [s for s in mapio.SAVE_STEPS if s <= frames]
    host_seq = [np.zeros((len(steps), 14, states[0].full_w, states[0].full_h), np.uint8) for _ in range(emax)]

    def host_on_step(i, act, predicted):
        if i + 1 in steps:
            for s in act:
                full_map = s.full_map.cpu().numpy() * 255                         # collect_maps.py:81-82
                host_seq[states.index(s)][steps.index(i + 1)] = full_map.astype(np.uint8)
    rec = mapio.MapSequenceRecorder(states, save_steps=steps)
    sides = {"none": None, "host": host_on_step, "device": rec.on_step}
    recs = []
    for E in batches:
        goals = [3] * E
        for name in sides:
            run_episodes(states[:E], [ep[:27] for ep in eps[:E]], goals, detector=det, on_step=sides[name])
        gc.collect()
        t = {name: [] for name in sides}
        for _ in range(repeats):
            for name in sides:
                if name == "device":
                    rec.reset()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run_episodes(states[:E], eps[:E], goals, detector=det, on_step=sides[name])
                if name == "device":
                    keeps = [rec.keep(s) for s in states[:E]]                     # the decision is part of the recorder's work
                elif name == "host":
                    keeps_host = [mapio.keep_sequence(q) for q in host_seq[:E]]
                torch.cuda.synchronize()
                t[name].append(E * frames / (time.perf_counter() - t0))
        same = all(np.array_equal(rec.sequence(s), host_seq[e]) for e, s in enumerate(states[:E]))
        ms = {name: 1e3 * E / _spread(t[name])["median"] for name in sides}
        r = {"section": "record_maps", "E": E, "frames": frames, "save_steps": steps,
             "no_recorder_steps_per_s": _spread(t["none"]), "host_recorder_steps_per_s": _spread(t["host"]),
             "device_recorder_steps_per_s": _spread(t["device"]),
             "ms_per_lockstep_step": {k: round(v, 3) for k, v in ms.items()},
             "recorder_adds_ms_per_save_step": {k: round((ms[k] - ms["none"]) * frames / len(steps), 3) for k in ("host", "device")},
             "sequences_equal": bool(same), "keep_equal": keeps == keeps_host, "launches": rec.launches}
        print(f"record maps, E = {E}: {r}", file=sys.stderr, flush=True)
        recs.append(r)
    return recs


def _goal_inputs(dev, n, frames=24, cache=None):
    """The goal-selection inputs of n episodes after `frames` frames of the pipeline's synthetic episodes: per episode
    (full_obstacle, collision_map, visited_vis, lmb, loc_rc) in the library's formats, and target_pred.  `cache`: a file to keep
    them in between processes that must see the same inputs."""
    if cache and os.path.exists(cache):
        items, tps = torch.load(cache)
        return [tuple(x.to(dev) if isinstance(x, torch.Tensor) else x for x in it) for it in items], [t.to(dev) for t in tps]
    from bench_pipeline import synth_episode
    from peanut_amd import goal as G
    from peanut_amd.agent_state import Agent_State, default_args
    from peanut_amd.prediction import PEANUT_Prediction_Model
    from peanut_amd.rcnn_weights import RcnnCfg, make_seeded_rcnn_state_dict
    from peanut_amd.replay import run_episode
    from peanut_amd.segmentation import HipDetector
    from peanut_amd.weights import PredCfg, make_seeded_state_dict
    args = default_args(only_explore=0, sem_gpu_id=dev.index, pred_precision="fp32", select_goal=True)
    model = PEANUT_Prediction_Model(args, state_dict=make_seeded_state_dict(PredCfg(), 0))
    rcfg = RcnnCfg(score_thresh_test=0.5)
    det = HipDetector(rcfg, make_seeded_rcnn_state_dict(rcfg, 0), device=dev)
    items, tps = [], []
    for e in range(n):
        ep = synth_episode(1000 + e, frames, dev)
        for fr in ep:
            for k in ("masks", "classes", "scores"):
                fr.pop(k)
        st = Agent_State(args, prediction_model=model)
        run_episode(st, ep, goal_cat=3, detector=det)
        st.full_map[:, st.lmb[0]:st.lmb[1], st.lmb[2]:st.lmb[3]] = st.local_map
        items.append((st.full_map[0].clone(), G._u8(st.collision_map, dev).clone(), G._u8(st.visited_vis, dev).clone(),
                      tuple(int(v) for v in st.lmb), (int(st.loc_r), int(st.loc_c))))
        tps.append(st.target_pred.float().clone())
    if cache:
        torch.save(([tuple(x.cpu() if isinstance(x, torch.Tensor) else x for x in it) for it in items], [t.cpu() for t in tps]), cache)
    return items, tps


def _maze_inputs(dev, n, size=960, window=480):
    """n seeded wall mazes in which the front crosses the whole map (the synthetic episodes' agent stands inside an obstacle:
    their fields end at once), agent cells and windows of one size at different places."""
    import numpy as np
    items, tps = [], []
    g = torch.Generator().manual_seed(0)
    for e in range(n):
        rng = np.random.RandomState(100 + e)
        ob = np.zeros((size, size), np.float32)
        for _ in range(int(0.012 * size * size / 20)):
            r, c, k = rng.randint(0, size), rng.randint(0, size), rng.randint(10, 60)
            if rng.rand() < 0.5:
                ob[r:r + 2, c:c + k] = 1
            else:
                ob[r:r + k, c:c + 2] = 1
        o = (size - window) // 2 + 10 * (e % 5) - 20
        loc = (200 + 7 * e, 260 - 5 * e)
        ob[o + loc[0] - 8:o + loc[0] + 9, o + loc[1] - 8:o + loc[1] + 9] = 0
        z = torch.zeros((size, size), dtype=torch.uint8, device=dev)
        items.append((torch.from_numpy(ob).to(dev), z, z.clone(), (o, o + window, o, o + window), loc))
        tps.append(torch.rand((window, window), generator=g).to(dev))
    return items, tps


def goal(dev, calls=10, repeats=3, cache=None, col_rad=None, mazes=False):
    from peanut_amd import goal as G
    from peanut_amd.agent_state import default_args
    args = default_args()
    rad = int(args.col_rad) if col_rad is None else col_rad
    T, res = float(getattr(args, "dist_weight_temperature", 500)), int(args.map_resolution)
    items, tps = _maze_inputs(dev, max(GOAL_BATCHES)) if mazes else _goal_inputs(dev, max(GOAL_BATCHES), cache=cache)
    H, W = items[0][0].shape
    has_batch = hasattr(G, "select_batch")
    out = {}
    for E in GOAL_BATCHES:
        seq = [G.GeodesicSolver(H, W, rad, device=dev) for _ in range(E)]
        bat = [G.GeodesicSolver(H, W, rad, device=dev) for _ in range(E)]
        last = {}

        def sequential(n):
            for _ in range(n):
                last["sequential"] = [s.select(*it, tp, T, res)["goal"] for s, it, tp in zip(seq, items, tps)]

        def sequential_begun(n):
            for _ in range(n):
                for s, it in zip(seq, items):
                    s.select_begin(*it)
                last["sequential_begun"] = [s.select(*it, tp, T, res)["goal"] for s, it, tp in zip(seq, items, tps)]

        def batch(n):
            for _ in range(n):
                last["batch"] = [r["goal"] for r in G.select_batch(bat, items[:E], tps[:E], T, res)]

        def batch_begun(n):
            for _ in range(n):
                G.select_begin_batch(bat, items[:E])
                last["batch_begun"] = [r["goal"] for r in G.select_batch(bat, items[:E], tps[:E], T, res)]
        sides = [("sequential", sequential), ("sequential_begun", sequential_begun)]
        if has_batch:
            sides += [("batch", batch), ("batch_begun", batch_begun)]
        for _, fn in sides:
            fn(3)
        t = {name: [] for name, _ in sides}
        for _ in range(repeats):
            for name, fn in sides:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(calls)
                torch.cuda.synchronize()
                t[name].append((time.perf_counter() - t0) / calls * 1e3)
        out[str(E)] = {name + "_ms_per_step": _spread(v) for name, v in t.items()}
        out[str(E)]["passes"] = [s.passes for s in seq]
        out[str(E)]["rounds_sequential"] = [s.rounds for s in seq]
        if has_batch:
            out[str(E)]["rounds_batch"] = bat[0].rounds
            out[str(E)]["goals_equal"] = bool(last["sequential"] == last["batch"] == last["batch_begun"])
            out[str(E)]["speedup_median"] = round(_spread(t["sequential"])["median"] / _spread(t["batch"])["median"], 3)
        print(f"goal{' (mazes)' if mazes else ''}, E = {E}: {out[str(E)]}", file=sys.stderr, flush=True)
    return out


def goal_trace_child(dev, E, cache=None):
    """What the profiler watches: E solvers on E copies of ONE map (they settle together, so the last rounds of a stage wake no
    tile of any episode), two warm-up select_batch calls, a pause, one select_batch."""
    from peanut_amd import goal as G
    from peanut_amd.agent_state import default_args
    args = default_args()
    items, tps = _maze_inputs(dev, 1)
    H, W = items[0][0].shape
    sols = [G.GeodesicSolver(H, W, int(args.col_rad), device=dev) for _ in range(E)]
    its = [tuple(x.clone() if isinstance(x, torch.Tensor) else x for x in items[0]) for _ in range(E)]
    for _ in range(2):
        G.select_batch(sols, its, [tps[0]] * E, 500.0, int(args.map_resolution))
    torch.cuda.synchronize()
    time.sleep(0.3)
    r = G.select_batch(sols, its, [tps[0]] * E, 500.0, int(args.map_resolution))
    torch.cuda.synchronize()
    print(json.dumps({"E": E, "rounds": r[0]["rounds"], "passes": r[0]["passes"]}), flush=True)


def goal_trace(out_dir, cache=None):
    """Per E = 1, 8, 16 one profiler run of `goal_trace_child`: round-kernel dispatches of the last select_batch against the rounds
    it reports, and the duration of a round in which no tile is awake (the shortest dispatches of the round kernel)."""
    res = {}
    for E in (1, 8, 16):
        tdir = os.path.join(out_dir, f"goal_trace_tmp_{E}")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tdir, "--", sys.executable, os.path.abspath(__file__),
               "--goal-trace-child", str(E)] + (["--goal-inputs", cache] if cache else [])
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240, text=True)
        except (OSError, subprocess.TimeoutExpired) as e:
            res[str(E)] = {"error": f"rocprofv3 did not run: {e}"}
            continue
        dbs = glob.glob(os.path.join(tdir, "**", "*.db"), recursive=True)
        if r.returncode != 0 or not dbs:
            res[str(E)] = {"error": f"rocprofv3 exit {r.returncode}, {len(dbs)} databases", "tail": r.stdout[-600:]}
            continue
        said = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith('{"E"')]
        rows = sqlite3.connect(dbs[0]).execute("select name, start, end from kernels order by start").fetchall()
        cut = max(range(1, len(rows)), key=lambda i: rows[i][1] - rows[i - 1][2])       # the pause
        ks = rows[cut:]
        rk = sorted((k[2] - k[1]) / 1e3 for k in ks if "fmm_round" in k[0])
        busy = sum(k[2] - k[1] for k in ks) / 1e3
        res[str(E)] = {"reported_rounds": said[-1]["rounds"] if said else None, "passes": said[-1]["passes"] if said else None,
                       "round_kernel_dispatches": len(rk), "kernels": len(ks),
                       "round_us_shortest_five": [round(x, 2) for x in rk[:5]], "round_us_median": round(rk[len(rk) // 2], 2) if rk else None,
                       "round_kernel_us_total": round(sum(rk), 1), "all_kernel_us": round(busy, 1),
                       "span_us": round((ks[-1][2] - ks[0][1]) / 1e3, 1)}
        import shutil
        shutil.rmtree(tdir, ignore_errors=True)
    res["note"] = ("one select_batch over E copies of one map, under the profiler (every launch is slower: the us show the split, not "
                   "the rate); the shortest round dispatches are rounds in which no tile of any episode is awake")
    return res


def trace_child(dev, E=8, steps=50):
    """What the profiler watches: warm-up, a pause, `steps` sequential steps of E episodes, a pause, `steps` batched steps."""
    sequential, batched, keep = _stage2_sides(E, dev)
    sequential(5)
    batched(5)
    for fn in (sequential, batched):
        torch.cuda.synchronize()
        time.sleep(0.3)                                            # a kernel-free pause in front of each timed part
        fn(steps)
    torch.cuda.synchronize()


def _summarise_trace(db_path, E, steps):
    db = sqlite3.connect(db_path)
    rows = db.execute("select name, start, end from kernels order by start").fetchall()
    # the two pauses are the two widest idle intervals of the trace: warm-up | sequential | batched
    cuts = sorted(sorted(range(1, len(rows)), key=lambda i: rows[i][1] - rows[i - 1][2])[-2:])
    parts = {"sequential": rows[cuts[0]:cuts[1]], "batched": rows[cuts[1]:]}
    res = {}
    for name, ks in parts.items():
        mapk = [k for k in ks if "map_" in k[0]]
        busy = sum(k[2] - k[1] for k in ks)
        gaps = sum(max(ks[i][1] - ks[i - 1][2], 0) for i in range(1, len(ks)))
        res[name] = {"steps": steps, "kernels_per_step": round(len(ks) / steps, 2),
                     "stage2_kernels_per_step": round(len(mapk) / steps, 2),
                     "kernel_us_per_step": round(busy / steps / 1e3, 2), "idle_gap_us_per_step": round(gaps / steps / 1e3, 2),
                     "span_us_per_step": round((ks[-1][2] - ks[0][1]) / steps / 1e3, 2)}
    res["note"] = (f"E = {E}; a step is E episodes; torch's own kernels (pose stack, copies) are in kernels_per_step, the library's "
                   "map_* kernels alone in stage2_kernels_per_step; under the profiler every launch is slower, so the us here "
                   "show the split between kernel time and gaps, not the rate")
    return res


def trace(out_dir, E=8, steps=50):
    tdir = os.path.join(out_dir, "trace_tmp")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tdir, "--", sys.executable, os.path.abspath(__file__), "--trace-child"]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240, text=True)
    except (OSError, subprocess.TimeoutExpired) as e:
        return {"error": f"rocprofv3 did not run: {e}"}
    dbs = glob.glob(os.path.join(tdir, "**", "*.db"), recursive=True)
    if r.returncode != 0 or not dbs:
        return {"error": f"rocprofv3 exit {r.returncode}, {len(dbs)} databases", "tail": r.stdout[-600:]}
    res = _summarise_trace(dbs[0], E, steps)
    import shutil
    shutil.rmtree(tdir, ignore_errors=True)                       # the database stays out of the repository; the summary is the record
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lockstep"))
    ap.add_argument("--no-pipeline", action="store_true")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--goal-only", action="store_true", help="the goal section alone")
    ap.add_argument("--pipeline-only", action="store_true", help="the pipeline section alone")
    ap.add_argument("--goalmap-only", action="store_true", help="the goalmap section alone -> <out>/goalmap.jsonl")
    ap.add_argument("--plan-stg", action="store_true",
                    help="the pipeline with the group's short-term goals after every step, batch_stg off and on -> <out>/plan_stg.jsonl")
    ap.add_argument("--plan-act", action="store_true",
                    help="the pipeline with the motor action (Agent_State_Group.plan_acts) off and on -> profiles/plan/lockstep_plan_act.jsonl")
    ap.add_argument("--visualize", action="store_true",
                    help="the plan_act pipeline with the visualisation frame off, on the device and on the host -> profiles/vis/lockstep_visualize.jsonl")
    ap.add_argument("--record-maps", action="store_true",
                    help="the pipeline with no recorder, a host recorder and mapio.MapSequenceRecorder -> profiles/mapio/recorder.jsonl")
    ap.add_argument("--pipeline-batches", default=",".join(str(b) for b in BATCHES))
    ap.add_argument("--goal-inputs", default=None, help="file that keeps the goal section's inputs between processes")
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--goal-trace-child", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    if a.trace_child:
        trace_child(dev)
        return
    if a.goal_trace_child:
        goal_trace_child(dev, a.goal_trace_child, cache=a.goal_inputs)
        return
    if a.record_maps:
        out = os.path.join(ROOT, "profiles", "mapio")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "recorder.jsonl"), "w") as f:
            for r in record_maps(dev):
                r["device"] = torch.cuda.get_device_name(dev)
                f.write(json.dumps(r) + "\n")
        return
    if a.visualize:
        out = os.path.join(ROOT, "profiles", "vis")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "lockstep_visualize.jsonl"), "w") as f:
            for r in visualize_pipeline(dev):
                r["device"] = torch.cuda.get_device_name(dev)
                f.write(json.dumps(r) + "\n")
        return
    if a.plan_act:
        out = os.path.join(ROOT, "profiles", "plan")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "lockstep_plan_act.jsonl"), "w") as f:
            for r in plan_act_pipeline(dev):
                r["device"] = torch.cuda.get_device_name(dev)
                f.write(json.dumps(r) + "\n")
        return
    os.makedirs(a.out, exist_ok=True)
    if a.goalmap_only:
        recs = goalmap(dev)
        if not a.no_pipeline:
            recs += goalmap_pipeline(dev)
        with open(os.path.join(a.out, "goalmap.jsonl"), "w") as f:
            for r in recs:
                r["device"] = torch.cuda.get_device_name(dev)
                f.write(json.dumps(r) + "\n")
        return
    if a.plan_stg:
        with open(os.path.join(a.out, "plan_stg.jsonl"), "w") as f:
            for r in stg_pipeline(dev):
                r["device"] = torch.cuda.get_device_name(dev)
                f.write(json.dumps(r) + "\n")
        return
    rec = {"device": torch.cuda.get_device_name(dev), "batches": list(BATCHES),
           "method": "one process; per E the two sides alternate, three repeats each; spread = min / median / max of the three"}
    pb = tuple(int(b) for b in a.pipeline_batches.split(","))
    if a.goal_only:
        rec["goal"] = goal(dev, cache=a.goal_inputs)
        rec["goal_mazes"] = goal(dev, mazes=True)
        if not a.no_trace:
            rec["goal_trace"] = goal_trace(a.out)
    elif a.pipeline_only:
        rec["pipeline"] = pipeline(dev, batches=pb)
    else:
        rec["forward_only"] = forward_only(dev)
        rec["stage2"] = stage2(dev)
        rec["goal"] = goal(dev, cache=a.goal_inputs)
        rec["goal_mazes"] = goal(dev, mazes=True)
        if not a.no_pipeline:
            rec["pipeline"] = pipeline(dev, batches=pb)
        if not a.no_trace:
            rec["trace"] = trace(a.out)
            rec["goal_trace"] = goal_trace(a.out)
    with open(os.path.join(a.out, "lockstep.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
