"""Cases of the batched short-term goal (peanut_stg_plan_batch; test infrastructure, importable without a GPU).

A batch takes episodes whose planners agree in m, the full map, col_rad and step size, so the cases of tests/stg_cases.py are sorted
into such groups here.  The m = 62, col_rad 0 group is completed by two new scenes so that it holds every chain ``_get_stg`` can take:

    serpentine_toilet     first solve + 2 magnify steps                        3 solves
    serpentine_chair      first solve + 8 magnify steps (the limit)            9
    serpentine_shortcut   first solve + 2 magnify steps, then near             3
    a04 (mask case)       random clutter, whatever the field gives
    plugged_corridor      first solve, eroded retry                            2
    plugged_serpentine    first solve, eroded retry, 8 magnify steps          10 (the longest chain there is)

Both new scenes follow ``blocked_start``: the walls are the COLLISION map, which the retry's erosion does not touch, the corridors are
one cell wide (the whole-cell margin of stg_cases needs that), and one isolated obstacle cell plugs the walk until the erosion
removes it.  tests/test_stg_batch_cpu.py holds their chains and margins on the oracle's field."""
import numpy as np

import stg_cases as sc

SERPENTINE = [(4, 4), (56, 4), (56, 20), (6, 20), (6, 36), (56, 36), (56, 52), (20, 52)]      # the walk of stg_cases' serpentine scenes


def new_scenes():
    out = []
    # blocked_start at m = 62, col_rad 0: nothing found, so the chain ends after the retry
    c = sc._scene("plugged_corridor", 62, "bottom", 0, (30.5, 12.5), 0, "bed", (12, 50), 1, 0)
    free = np.zeros((62, 62), bool)
    sc._carve(free, [(30, 4), (30, 33), (12, 33), (12, 50)])
    sc._local(c, "collision")[~free] = 1
    c["obstacle"][30, 25] = 0.500001
    out.append(c)
    # the serpentine of stg_cases with its walls in the collision map and a plug in the first lane: the retry opens the walk, the
    # found chair at its end is still farther than 100 cells, and the eight magnify steps leave it there
    c = sc._scene("plugged_serpentine", 62, "bottom", 0, (10.5, 4.5), 1, "chair", (20, 52), 1, 8)
    free = np.zeros((62, 62), bool)
    sc._carve(free, SERPENTINE)
    sc._local(c, "collision")[~free] = 1
    c["obstacle"][40, 4] = 1.5
    out.append(c)
    return out


def group_key(c):
    return (c["m"], c["full"], c["col_rad"])


def groups():
    """{(m, full, col_rad): [cases]} over the scenes and mask cases of stg_cases plus the new scenes, in a fixed order."""
    out = {}
    for c in sc.scene_cases() + new_scenes() + sc.mask_cases():
        out.setdefault(group_key(c), []).append(c)
    return out


FULL_GROUP = (62, 124, 0)       # n = 64: 2 x 2 solver tiles exactly; E = 6, every chain
PAIR_GROUP = (61, 122, 1)       # n = 63: blocked_start (retry) + a09; E = 2
TRIPLE_GROUP = (61, 122, 0)     # n = 63: doors + a00 + a12; E = 3
RAGGED_GROUP = (45, 90, 1)      # n = 47: unreachable + a05, the seeds of the E = 16 batch


def variants16():
    """Sixteen episodes at m = 45, col_rad 1 from the two cases of that group with other starts and goals: the closed room seen from
    along its corridor (found and not, toilet and chair: retry with and without magnify steps), goals ON the corridor (plain), and the
    cluttered mask case from eight starts."""
    by = {c["name"]: c for c in groups()[RAGGED_GROUP]}
    room = by["unreachable"]
    clutter = next(c for n, c in by.items() if n.startswith("a05"))
    out = []
    for k, (col, found, name, goal_cell) in enumerate([(12, 1, "toilet", (32, 30)), (20, 0, "chair", (32, 30)), (30, 1, "chair", (30, 36)),
                                                        (36, 1, "toilet", (8, 8)), (8, 0, "bed", (8, 36)), (16, 1, "chair", (8, 37)),
                                                        (26, 0, "toilet", (26, 38)), (34, 1, "bed", (40, 24))]):
        c = dict(room, name=f"room_{k}", start_exact=[8.5, col + 0.25 * (k % 4)], found_goal=found, goal_name=name)
        c["goal"] = np.zeros_like(room["goal"])
        c["goal"][goal_cell] = 1
        out.append(c)
    for k, (r, col) in enumerate([(3, 3), (10, 30), (22, 22), (40, 5), (5, 40), (30, 12), (41, 41), (17, 36)]):
        c = dict(clutter, name=f"clutter_{k}", start_exact=[r + 0.5, col + 0.125 * k], found_goal=k % 2, goal_name=("chair", "toilet")[k // 4])
        if k >= 4:
            c["goal"] = np.roll(clutter["goal"], (3 * k, 5 * k), (0, 1))
        out.append(c)
    return out
