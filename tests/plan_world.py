"""A toy kinematic world that closes the agent loop around ``Agent_Helper.plan_act`` (test infrastructure; the world itself needs no
GPU): a 120 x 120-cell map of 5 cm cells under ``global_downscaling = 1`` (one window over the whole map), forward steps of 0.25 m,
turns of 30 degrees.  A forward move whose path meets an occupied world cell leaves the pose unchanged (a bump).  The planner
inputs are built from the world directly -- no perception: the obstacle plane is the world's walls WITHOUT its "glass" cells, which
block motion but which no sensor sees; the goal plane is the goal blob, found from the first step.

Conventions (nav/agent/agent_helper.py:257-268, :304-312, :348-363): the pose is (x, y, o) in metres and degrees, x along the
columns, y along the rows, o counter-clockwise from +x towards +y; action 1 moves forward, 2 turns left (o + 30), 3 right (o - 30),
0 stops."""
import math
from types import SimpleNamespace

import numpy as np

N = 120                       # cells per side
RES = 5                       # cm per cell
FORWARD_M = 0.25
TURN_DEG = 30.0
COL_RAD = 4
MIN_CORRIDOR = 2 * COL_RAD + 3
LMB = [0, N, 0, N]
SUCCESS_M = 1.0               # the ObjectNav success radius


def world_args(**over):
    a = dict(map_size_cm=N * RES, map_resolution=RES, global_downscaling=1, num_sem_categories=10, col_rad=COL_RAD, only_explore=0,
             move_forward_after_stop=1, turn_angle=TURN_DEG, collision_threshold=0.20, magnify_goal_when_hard=100, visualize=0)
    a.update(over)
    return SimpleNamespace(**a)


class World:
    def __init__(self, walls, glass, goal, pose):
        self.walls, self.glass, self.goal = walls.astype(bool), glass.astype(bool), goal.astype(bool)
        self.blocked = self.walls | self.glass
        self.pose = [float(v) for v in pose]
        self.bumps = 0
        assert not self.blocked[self.cell()], "the agent starts inside a wall"

    def cell(self, x=None, y=None):
        x, y = (self.pose[0], self.pose[1]) if x is None else (x, y)
        return int(y * 100.0 / RES), int(x * 100.0 / RES)

    def step(self, action):
        """The world's answer to an action; returns whether the pose changed."""
        x, y, o = self.pose
        if action == 2:
            self.pose[2] = o + TURN_DEG
        elif action == 3:
            self.pose[2] = o - TURN_DEG
        elif action == 1:
            dx, dy = FORWARD_M * math.cos(math.radians(o)), FORWARD_M * math.sin(math.radians(o))
            for k in range(1, 11):                      # the path in half-cell steps: no wall is jumped
                r, c = self.cell(x + dx * k / 10, y + dy * k / 10)
                if not (0 <= r < N and 0 <= c < N) or self.blocked[r, c]:
                    self.bumps += 1
                    return False
            self.pose[0], self.pose[1] = x + dx, y + dy
        return action != 0

    def distance_to_goal_m(self):
        r, c = self.cell()
        gr, gc = np.nonzero(self.goal)
        return float(np.sqrt((gr - r) ** 2 + (gc - c) ** 2).min()) * RES / 100.0

    def planner_inputs(self, device=None):
        """The dict ``plan_act`` takes; with ``device`` the maps are HIP tensors (made once per world)."""
        if device is None:
            obstacle, goal = self.walls.astype(np.float32), self.goal.astype(np.float64)
        else:
            import torch
            if getattr(self, "_dev", None) is None:
                self._dev = (torch.from_numpy(self.walls.astype(np.float32)).to(device), torch.from_numpy(self.goal.astype(np.uint8)).to(device))
            obstacle, goal = self._dev
        return {'obstacle': obstacle, 'exp_pred': None, 'goal': goal, 'pose_pred': np.array(self.pose + LMB, np.float64), 'found_goal': 1,
                'goal_name': 'chair'}


def corridor_widths(walls):
    """The lengths of all maximal free runs along rows and along columns (the border walls excluded)."""
    runs = []
    for grid in (walls, walls.T):
        for line in grid[1:-1]:
            free = np.concatenate(([0], (~line[1:-1]).astype(np.int8), [0]))
            edges = np.flatnonzero(np.diff(free))
            runs += list(edges[1::2] - edges[::2])
    return runs


GLASS = (slice(12, 23), 30)     # eleven cells across the straight line from the start to the near door


def maze(glass):
    """Three rooms behind walls three cells thick.  Wall A (columns 40..42) has a door near the start (rows 12..22) and a second one
    far down (rows 90..104); wall B (columns 78..80) has one door (rows 60..74); the goal blob lies in the last room.  ``glass``: a
    pane stands in the open floor of the first room, across the way to the near door -- the agent has to feel its way round it."""
    walls = np.zeros((N, N), bool)
    walls[0], walls[-1], walls[:, 0], walls[:, -1] = True, True, True, True
    walls[:, 40:43] = True
    walls[12:23, 40:43] = False
    walls[90:105, 40:43] = False
    walls[:, 78:81] = True
    walls[60:75, 78:81] = False
    walls[0], walls[-1] = True, True
    pane = np.zeros((N, N), bool)
    if glass:
        pane[GLASS] = True
    goal = np.zeros((N, N), bool)
    goal[99:102, 99:102] = True
    return World(walls, pane, goal, (1.025, 0.875, 0.0))       # cell (17, 20), facing the near door


def state_stand_in(args, device="cuda:0"):
    """What ``Agent_Helper`` needs of an ``Agent_State`` (no mapping module, no prediction model): the two planner-side maps on the
    device, the short-term-goal planner, the preset counter."""
    import torch
    from peanut_amd.planner import ShortTermGoal
    full = int(args.map_size_cm // args.map_resolution)
    st = SimpleNamespace(args=args, device=torch.device(device), stg=None, stg_stop=None, helper=None, presets=0, _stg=None,
                         collision_map=torch.zeros((full, full), dtype=torch.uint8, device=device),
                         visited_vis=torch.zeros((full, full), dtype=torch.uint8, device=device))

    def planner():
        if st._stg is None:
            st._stg = ShortTermGoal(args, device=device)
        return st._stg

    def next_preset_goal():
        st.presets += 1

    st._stg_planner, st.next_preset_goal = planner, next_preset_goal
    return st


def run_episode(helper, world, max_steps, device=None):
    """plan_act -> world.step until action 0 or ``max_steps`` -> (actions, poses)."""
    actions, poses = [], []
    for _ in range(max_steps):
        a = helper.plan_act(world.planner_inputs(device))['action']
        actions.append(int(a))
        poses.append(tuple(world.pose))
        if a == 0:
            break
        world.step(a)
    return actions, poses
