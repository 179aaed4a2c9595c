"""The agent loop closed in a toy kinematic world (tests/plan_world.py): ``Agent_Helper.plan_act`` with the real device short-term
goal -> an action -> the world moves the agent (or does not: a bump) -> the next planner inputs.

(i)  A wall maze with the goal blob visible: the episode ends with action 0 within 150 steps, the agent within 1 m of the blob (the
     ObjectNav success radius: a condition of the task, not a measurement).
(ii) The same maze with a pane of "glass" that blocks motion and is absent from the obstacle map: the agent bumps, ``collision_map``
     becomes non-zero at the pane, and the agent still reaches the goal within 300 steps -- the path through goal selection and the
     short-term goal that nothing could reach while no product code wrote the planner-side maps.

The corridors and doors are at least ``2 * col_rad + 3`` cells wide, so that the outcome does not hinge on the solver's last half
cell.  With the reference's planner arithmetic (oracle field, NumPy window) the two episodes take 30 and 75 steps."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import plan_world as pw
from peanut_amd.agent_helper import Agent_Helper

pytestmark = pytest.mark.gpu


def _episode(glass, max_steps):
    args = pw.world_args()
    state = pw.state_stand_in(args)
    helper = Agent_Helper(args, state)
    helper.reset()
    world = pw.maze(glass)
    np.random.seed(0)
    actions, poses = pw.run_episode(helper, world, max_steps, device=state.device)
    torch.cuda.synchronize()
    print(f"world glass={glass}: {len(actions)} steps, {world.bumps} bumps, {world.distance_to_goal_m():.2f} m from the goal, "
          f"{int(state.collision_map.sum())} collision cells; actions {''.join(str(a) for a in actions)}")
    return helper, state, world, actions, poses


def test_the_maze_is_as_wide_as_the_planner_needs():
    for glass in (False, True):
        w = pw.maze(glass)
        assert min(pw.corridor_widths(w.walls)) >= pw.MIN_CORRIDOR
        assert w.glass.sum() == (11 if glass else 0) and not (w.glass & w.walls).any()


def test_wall_maze_ends_with_stop_near_the_goal():
    helper, state, world, actions, poses = _episode(False, 150)
    assert actions[-1] == 0, f"no stop within 150 steps (the last pose is {world.pose})"
    assert world.distance_to_goal_m() <= pw.SUCCESS_M
    assert (world.bumps == 0) == (int(state.collision_map.sum()) == 0)          # cells are marked by bumps and by nothing else
    # the visited line follows the agent: every cell it stood on is marked (none lies on row or column 0)
    vis = state.visited_vis.cpu().numpy()
    assert all(vis[world.cell(x, y)] == 1 for x, y, _ in poses)
    assert helper.timestep == len(actions)


def test_glass_is_felt_marked_and_walked_around():
    helper, state, world, actions, poses = _episode(True, 300)
    assert world.bumps > 0
    col = state.collision_map.cpu().numpy()
    rows, c = pw.GLASS
    near = np.zeros_like(col, bool)
    near[rows.start - 6:rows.stop + 6, c - 6:c + 7] = True             # buf + length cells ahead of an agent that stands before the pane
    assert col[near].sum() > 0, "no collision cell at the glass"
    assert actions[-1] == 0, f"no stop within 300 steps (the last pose is {world.pose})"
    assert world.distance_to_goal_m() <= pw.SUCCESS_M
