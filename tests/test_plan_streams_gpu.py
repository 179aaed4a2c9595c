"""The stream contract of the planner's mark (include/peanut_hip.h: "enqueued on maps->stream, no synchronisation") with the
protocols of tests/stream_cases.py.  The two entries take their stream in a struct, like peanut_stg_plan_batch and the map-dataset
calls, so they are held here and not in the prototype table of tests/test_streams_cpu.py.

* P1 on ``peanut_plan_mark`` and ``peanut_plan_mark_batch`` (E = 3): the maps are overwritten late behind a backlog and again right
  after the call; the marked maps equal those of the idle default stream, and the call returns while the backlog is pending.
* P1 (without the pending assertion: the short-term goal synchronises) on mark + ``ShortTermGoal.get_stg`` enqueued on a side
  stream: the short-term goal sees the cell the mark of the same step set -- the result equals the serial order, and differs from
  the one without the mark."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import stream_cases as sc
from peanut_amd.agent_helper import plan_mark, plan_mark_batch

pytestmark = pytest.mark.gpu

FULL = 64
MARKS = [((8, 40, 16, 48), (3, 30), (29, 0), [(0, 0), (63, 63), (20, 41)]),
         ((0, 32, 0, 32), (31, 31), (0, 9), []),
         ((32, 64, 32, 64), (7, 7), (7, 7), [(r, 2 * r) for r in range(28)])]


def _maps(E):
    """seed -> 2 E uint8 [FULL, FULL] maps with a random 0 / 1 pattern (a mark only sets cells: what was there shows through)."""
    def build(seed):
        g = torch.Generator().manual_seed(977 * seed + 5)
        return tuple((torch.rand((FULL, FULL), generator=g) < 0.25).to(torch.uint8) for _ in range(2 * E))
    return build


def test_mark_single_and_batched_behind_a_backlog():
    def single(h, x, outs):
        maps = [t.clone() for t in x]                 # (stream-ordered copies: the inputs stay as they are)
        plan_mark(maps[0], maps[1], *MARKS[0])
        return maps
    sc.p1("peanut_plan_mark", lambda: None, single, sc.to_device(_maps(1)(0)), sc.to_device(_maps(1)(1)), "async")

    def batch(h, x, outs):
        maps = [t.clone() for t in x]
        plan_mark_batch([(maps[2 * e], maps[2 * e + 1]) + MARKS[e] for e in range(3)])
        return maps
    sc.p1("peanut_plan_mark_batch", lambda: None, batch, sc.to_device(_maps(3)(0)), sc.to_device(_maps(3)(1)), "async")


def test_mark_then_short_term_goal_on_a_side_stream_equals_the_serial_order():
    import stg_cases
    from peanut_amd.planner import ShortTermGoal
    c = next(s for s in stg_cases.scene_cases() if s["name"] == "blocked_start")
    args = SimpleNamespace(map_size_cm=c["full"] * 5, map_resolution=5, global_downscaling=2, col_rad=c["col_rad"],
                           magnify_goal_when_hard=stg_cases.MAGNIFY_WHEN_HARD)
    gx1, _, gy1, _ = c["lmb"]
    start = (int(c["start_exact"][0]), int(c["start_exact"][1]))
    cell = (gx1 + 30, gy1 + 16)                       # on the one-cell walk ahead of the agent: the way is shut once it is marked

    def run(p, x, outs, mark=True):
        collision, visited = x[2].clone(), x[3].clone()       # (stream-ordered copies: the inputs stay as they are)
        if mark:
            plan_mark(visited, collision, c["lmb"], (start[0], 4), start, [cell])
        p.get_stg(x[0], x[1], collision, visited, c["lmb"], c["start_exact"], c["found_goal"], c["goal_name"], taps=True)
        return dict(p.last, visited=visited, collision=collision)
    make = lambda: ShortTermGoal(args, device="cuda:0")  # noqa: E731
    good, stale = sc.to_device(sc.INPUTS["stg_scenes"](0)), sc.to_device(sc.INPUTS["stg_scenes"](1))
    p = sc.p1("plan_mark + peanut_stg_plan", make, run, good, stale, "syncs")
    without = run(p, good, None, mark=False)
    with_mark = run(p, good, None)
    torch.cuda.synchronize()
    assert int(with_mark["collision"][cell]) == 1 and int(without["collision"][cell]) == 0
    assert with_mark["distance"] != without["distance"], "the marked cell does not reach the short-term goal: the case cannot tell the order"
    assert np.array_equal(with_mark["visited"].cpu().numpy()[gx1 + start[0] - 1:gx1 + start[0] + 1, gy1 + 3:gy1 + start[1] + 1],
                          np.ones((2, start[1] - 2), np.uint8))
