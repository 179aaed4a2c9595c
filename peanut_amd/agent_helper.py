"""The reference's ``Agent_Helper`` (nav/agent/agent_helper.py), device-resident where it is heavy.

* Observation formatting (:166-217): ``preprocess_obs`` produces the ``[1, 4+ncat, h, w]`` tensor that ``Semantic_Mapping``
  consumes, with one HIP launch (``peanut_preprocess_obs``) instead of the reference's per-column Python loop on the host.
* Motion planning (:19-48, :51-159, :228-371): ``Agent_Helper`` / ``UnTrapHelper`` with the reference's surface -- ``reset``,
  ``set_goal_cat``, ``plan_act(planner_inputs) -> {'action': a}``, ``_plan``.  The scalar state machine (collision test, stop
  countdown, angle arithmetic, untrap) runs on the host in the reference's own number types; what touches a map does not: the
  visited line and the collision cells go into ``Agent_State.visited_vis`` / ``collision_map`` where they lie on the device in one
  launch (``peanut_plan_mark``, csrc/plan.hip), and the short-term goal comes from ``planner.ShortTermGoal`` (csrc/stg.hip).
  ``plan_act_batch`` is the lock-step form: E marks in one ``peanut_plan_mark_batch``, E short-term goals in one
  ``get_stg_batch``, every action, counter and map the bits of E single calls.
* Visualisation (:496-621): with ``args.visualize`` non-zero ``plan_act`` ends with ``_visualize`` (:154-155), which renders the
  reference's ``vis_image`` on the device (``peanut_amd.vis.VisRenderer``, csrc/vis.hip: three launches, one read-back) and, with
  ``visualize == 2``, writes it under the reference's file name (PIL, JPEG quality 100).  With ``visualize == 1`` the frame is
  kept in ``self.vis_image`` and NO window opens (a deviation: no cv2 here).  ``plan_act_batch`` renders its episodes in one
  ``render_batch``.  Not here: ``use_gt_seg`` (dead code in the reference: it reads ``sem_seg_pred`` before assigning it).

There is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib


def preprocess_obs(rgb: torch.Tensor, depth: torch.Tensor, sem_seg_pred: torch.Tensor, args) -> torch.Tensor:
    """``_preprocess_obs`` + ``_preprocess_depth``: rgb uint8 [H,W,3], depth float32 [H,W,1] or [H,W]
    (simulator units in [0,1], 0 = invalid), sem_seg_pred float32 [H,W,ncat] -- all HIP tensors --
    -> float32 [1, 3+1+ncat, frame_height, frame_width].  ``args``: env_frame_width, frame_width,
    min_depth, max_depth (nav/arguments.py:44-66)."""
    lib = _lib.load()
    if not (rgb.is_cuda and depth.is_cuda and sem_seg_pred.is_cuda):
        raise _lib.PeanutHipError("preprocess_obs needs HIP tensors (no CPU fallback)")
    if depth.dim() == 3:
        depth = depth[:, :, 0]
    H, W = depth.shape
    ds = args.env_frame_width // args.frame_width          # agent_helper.py:185
    ncat = sem_seg_pred.shape[2]
    rgb = rgb.to(torch.uint8).contiguous()
    depth = depth.to(torch.float32).contiguous()
    sem = sem_seg_pred.to(torch.float32).contiguous()
    obs = torch.empty((1, 4 + ncat, H // ds, W // ds), dtype=torch.float32, device=depth.device)
    with torch.cuda.device(depth.device):
        rc = lib.peanut_preprocess_obs(rgb.data_ptr(), depth.data_ptr(), sem.data_ptr(), H, W, ncat, ds,
                                       float(args.min_depth), float(args.max_depth), obs.data_ptr(),
                                       _lib.current_stream_ptr(depth.device))
    _lib.check(rc, "peanut_preprocess_obs")
    return obs


def preprocess_obs_batch(rgb: torch.Tensor, depth: torch.Tensor, sem_seg_pred: torch.Tensor, args) -> torch.Tensor:
    """``preprocess_obs`` for E frames in one launch (``peanut_preprocess_obs_batch``): rgb uint8 [E,H,W,3], depth float32
    [E,H,W,1] or [E,H,W], sem_seg_pred float32 [E,H,W,ncat] -> float32 [E, 3+1+ncat, frame_height, frame_width]; frame e has
    the bits ``preprocess_obs`` gives for it."""
    lib = _lib.load()
    if not (rgb.is_cuda and depth.is_cuda and sem_seg_pred.is_cuda):
        raise _lib.PeanutHipError("preprocess_obs_batch needs HIP tensors (no CPU fallback)")
    if depth.dim() == 4:
        depth = depth[:, :, :, 0]
    if depth.dim() != 3 or rgb.dim() != 4 or sem_seg_pred.dim() != 4:
        raise ValueError("preprocess_obs_batch takes rgb [E,H,W,3], depth [E,H,W(,1)], sem [E,H,W,ncat]")
    E, H, W = depth.shape
    ncat = sem_seg_pred.shape[3]
    if tuple(rgb.shape) != (E, H, W, 3) or tuple(sem_seg_pred.shape[:3]) != (E, H, W):
        raise ValueError(f"preprocess_obs_batch: rgb {tuple(rgb.shape)} / sem {tuple(sem_seg_pred.shape)} do not match depth {tuple(depth.shape)}")
    ds = args.env_frame_width // args.frame_width          # agent_helper.py:185
    rgb = rgb.to(torch.uint8).contiguous()
    depth = depth.to(torch.float32).contiguous()
    sem = sem_seg_pred.to(torch.float32).contiguous()
    obs = torch.empty((E, 4 + ncat, H // ds, W // ds), dtype=torch.float32, device=depth.device)
    with torch.cuda.device(depth.device):
        rc = lib.peanut_preprocess_obs_batch(rgb.data_ptr(), depth.data_ptr(), sem.data_ptr(), E, H, W, ncat, ds,
                                             float(args.min_depth), float(args.max_depth), obs.data_ptr(),
                                             _lib.current_stream_ptr(depth.device))
    _lib.check(rc, "peanut_preprocess_obs_batch")
    return obs


# ---------------------------------------------------------------------------------------------------------------------------------
# the planner's map bookkeeping on the device (csrc/plan.hip)
# ---------------------------------------------------------------------------------------------------------------------------------
def plan_line(last_start, start) -> np.ndarray:
    """``peanut_plan_line``: the 26 points of ``vu.draw_line(last_start, start, .)`` (utils/visualization.py:19-24) as the library
    computes them on the host -> int [26, 2].  Needs no device."""
    a, b = (C.c_int * 2)(int(last_start[0]), int(last_start[1])), (C.c_int * 2)(int(start[0]), int(start[1]))
    out = ((C.c_int * 2) * _lib.PLAN_LINE_POINTS)()
    _lib.check(_lib.load().peanut_plan_line(C.byref(a), C.byref(b), C.byref(out)), "peanut_plan_line")
    return np.array([[p[0], p[1]] for p in out], dtype=np.int64)


def _mark_struct(visited_vis, collision_map, lmb, last_start, start, cells):
    cells = [(int(r), int(c)) for r, c in cells]
    if len(cells) > _lib.PLAN_MAX_CELLS:
        raise ValueError(f"at most {_lib.PLAN_MAX_CELLS} collision cells per step, got {len(cells)}")
    ep = _lib.PlanMarkC(visited_vis=visited_vis.data_ptr(), collision_map=collision_map.data_ptr(), n_cells=len(cells))
    ep.lmb[:] = [int(v) for v in lmb]
    ep.last_start[:] = [int(v) for v in last_start]
    ep.start[:] = [int(v) for v in start]
    for k, (r, c) in enumerate(cells):
        ep.cells_rc[k][0], ep.cells_rc[k][1] = r, c
    return ep


def plan_mark_batch(marks) -> None:
    """``peanut_plan_mark_batch`` (E = 1: ``peanut_plan_mark``): one launch on the current stream for E episodes.  ``marks``: E tuples
    ``(visited_vis, collision_map, lmb, last_start, start, cells)`` -- the two maps uint8 [full_w, full_h] contiguous HIP tensors of
    one shape and device, written where they lie; ``lmb`` the m x m window; ``last_start`` / ``start`` window cells in [0, m);
    ``cells`` up to 28 full-map ``(r, c)`` pairs.  ``ValueError`` for what the tensors' own metadata shows, ``PeanutHipError`` for what
    the library refuses (nothing is enqueued then and every map is as it was)."""
    marks = [tuple(mk) for mk in marks]
    E = len(marks)
    if E < 1 or E > _lib.PLAN_MAX_BATCH:
        raise ValueError(f"plan_mark_batch takes 1..{_lib.PLAN_MAX_BATCH} episodes, got {E}")
    v0 = marks[0][0]
    for e, mk in enumerate(marks):
        if len(mk) != 6:
            raise ValueError("plan_mark_batch needs (visited_vis, collision_map, lmb, last_start, start, cells) per episode")
        for name, t in (("visited_vis", mk[0]), ("collision_map", mk[1])):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8 or t.dim() != 2 or not t.is_contiguous():
                raise ValueError(f"episode {e}: {name} must be a contiguous 2-D uint8 HIP tensor (no CPU fallback)")
            if t.shape != v0.shape or t.device != v0.device:
                raise ValueError(f"episode {e}: {name} is {tuple(t.shape)} on {t.device}, episode 0's maps are {tuple(v0.shape)} on {v0.device}")
        if len(mk[2]) != 4 or len(mk[3]) != 2 or len(mk[4]) != 2:
            raise ValueError(f"episode {e}: lmb holds four boundaries, last_start and start two cells")
    eps = (_lib.PlanMarkC * E)(*[_mark_struct(*mk) for mk in marks])
    lib = _lib.load()
    with torch.cuda.device(v0.device):
        maps = _lib.PlanMapsC(full_w=int(v0.shape[0]), full_h=int(v0.shape[1]), stream=_lib.current_stream_ptr(v0.device))
        if E == 1:
            rc, what = lib.peanut_plan_mark(C.byref(maps), C.byref(eps[0])), "peanut_plan_mark"
        else:
            rc, what = lib.peanut_plan_mark_batch(C.byref(maps), E, eps), "peanut_plan_mark_batch"
    _lib.check(rc, what)


def plan_mark(visited_vis, collision_map, lmb, last_start, start, cells=()) -> None:
    """``peanut_plan_mark``: ``visited_vis[gx1:gx2, gy1:gy2] = vu.draw_line(last_start, start, ...)`` (agent_helper.py:278-280) and
    ``collision_map[r, c] = 1`` for ``cells`` (:315) in one launch on the current stream; see ``plan_mark_batch``."""
    plan_mark_batch([(visited_vis, collision_map, lmb, last_start, start, cells)])


# ---------------------------------------------------------------------------------------------------------------------------------
# the motion planner's state machine (host) around them
# ---------------------------------------------------------------------------------------------------------------------------------
def _threshold(cell, shape):
    """``pu.threshold_poses`` (utils/pose.py:39-42)."""
    return [min(max(0, cell[0]), shape[0] - 1), min(max(0, cell[1]), shape[1] - 1)]


class UnTrapHelper:
    """The brute-force untrap sequence (agent_helper.py:19-48): while the agent is blocked, turn to one side for two tries, to the
    other for sixteen, back for twelve, then at random; the sides swap with every new block (``total_id``)."""

    def __init__(self):
        self.total_id = 0
        self.epi_id = 0

    def reset(self, full=False):                                    # :24-28
        self.total_id = 0 if full else self.total_id + 1
        self.epi_id = 0

    def get_action(self):                                           # :30-48
        self.epi_id += 1
        if self.epi_id > 30:
            return np.random.randint(2, 4)                          # the global RNG, as the reference
        first = 2 if self.total_id % 2 == 0 else 3
        if self.epi_id > 18 or self.epi_id < 3:
            return first
        return 5 - first


class Agent_Helper:
    """The planning half of the reference's ``Agent_Helper`` (agent_helper.py:51-159, :228-371).  ``collision_map`` and
    ``visited_vis`` ARE the ``Agent_State`` tensors (uint8 HIP, [full_w, full_h]): this class is their writer, goal selection and the
    short-term goal their readers.  ``agent_states.helper`` is set to this object (peanut_agent.py:24)."""

    def __init__(self, args, agent_states, rank=0, legend=None):
        self.args = args
        self.agent_states = agent_states
        agent_states.helper = self
        self.rank = rank
        self.legend = legend                    # an array or a path (agent_helper.py:102), read when the first frame is rendered
        self.rgb_vis = None                     # this step's uint8 RGB frame [480, 640, 3] (:222 keeps it as BGR; the device flips)
        self.vis_image = None
        self._vis = None
        self.collision_map = agent_states.collision_map
        self.visited_vis = agent_states.visited_vis
        self.col_width = None
        self.curr_loc = None
        self.last_loc = None
        self.last_action = None
        self.count_forward_actions = None
        self.last_start = None
        self.episode_no = 0
        self.stg = None
        self.goal_cat = -1
        self.goal_name = None
        self.found_goal = None
        self.untrap = UnTrapHelper()
        # one extra step forward after the stop condition, to end nearer the goal (:89-91)
        self.forward_after_stop_preset = self.args.move_forward_after_stop
        self.forward_after_stop = self.forward_after_stop_preset
        self.map_size = args.map_size_cm // args.map_resolution                       # :93-96
        self.full_w, self.full_h = self.map_size, self.map_size
        self.local_w = int(self.full_w / args.global_downscaling)
        self.local_h = int(self.full_h / args.global_downscaling)
        self.edge_buffer = 10 if args.num_sem_categories <= 16 else 40                # :99

    # ---- agent_helper.py:106-127 ----
    def reset(self):
        args = self.args
        self.collision_map = self.agent_states.collision_map
        self.visited_vis = self.agent_states.visited_vis
        self.collision_map.zero_()
        self.visited_vis.zero_()
        self.col_width = 1
        self.count_forward_actions = 0
        self.curr_loc = [args.map_size_cm / 100.0 / 2.0, args.map_size_cm / 100.0 / 2.0, 0.]
        self.last_action = None
        self.episode_no += 1
        self.timestep = 0
        self.prev_blocked = 0
        self._previous_action = -1
        self.block_threshold = 4
        self.untrap.reset(full=True)
        self.forward_after_stop = self.forward_after_stop_preset

    def set_goal_cat(self, goal_cat):                               # :162-163
        self.goal_cat = goal_cat

    # ---- agent_helper.py:130-159 ----
    def plan_act(self, planner_inputs):
        """``planner_inputs``: the dict of ``Agent_State.planner_inputs`` -- ``host=False`` (device views, nothing copied) is the
        cheap form; NumPy maps are uploaded.  Returns ``{'action': a}``: 0 stop, 1 forward, 2 left, 3 right."""
        self.timestep += 1
        self.goal_name = planner_inputs['goal_name']
        action = self._plan(planner_inputs)
        if getattr(self.args, "visualize", 0):                      # :154-155
            self._visualize(planner_inputs)
        self.last_action = action
        return {'action': action}

    # ---- agent_helper.py:496-621 ----
    def _renderer(self):
        if self._vis is None:
            from .vis import VisRenderer
            self._vis = VisRenderer(self.args, self.agent_states.device, legend=self.legend)
        return self._vis

    def _visualize(self, planner_inputs):
        """Render this step's frame on the device and keep it in ``self.vis_image`` (uint8 NumPy [600, 1415, 3], BGR)."""
        vis = self._renderer()
        vis.render(**self.agent_states.vis_item(planner_inputs, stg=self.stg, rgb=self.rgb_vis))
        self._keep_frame(vis.frame_host()[0])

    def _keep_frame(self, frame):
        self.vis_image = frame = np.array(frame)                     # out of the renderer's pinned buffer: it outlives the step
        if self.args.visualize == 2:                                 # :615-621
            import os
            from .vis import frame_path, write_frame
            ep_dir, fn = frame_path(self.args, self.rank, self.episode_no, self.timestep)
            os.makedirs(ep_dir, exist_ok=True)
            write_frame(fn, frame)

    def _plan(self, planner_inputs):
        """(:228-371) one ``peanut_plan_mark``, one short-term goal, the action."""
        step = self._plan_begin(planner_inputs)
        plan_mark_batch([step['mark']])
        stg, stop = self._get_stg(planner_inputs, step)
        return self._plan_end(planner_inputs, step, stg, stop)

    def _plan_begin(self, planner_inputs):
        """(:246-320) everything before ``_get_stg``: poses, cells, the collision test and its counters.  Returns the step's
        ``start`` / ``start_exact`` / ``lmb`` and ``mark``, the arguments of ``plan_mark`` (the maps are not touched here)."""
        args = self.args
        res = args.map_resolution
        self.last_loc = self.curr_loc                                                  # :248
        self.found_goal = planner_inputs['found_goal']
        shape = tuple(int(v) for v in planner_inputs['obstacle'].shape)               # map_pred.shape
        start_x, start_y, start_o, gx1, gx2, gy1, gy2 = planner_inputs['pose_pred']   # :257-259
        gx1, gx2, gy1, gy2 = int(gx1), int(gx2), int(gy1), int(gy2)
        self.curr_loc = [start_x, start_y, start_o]                                   # :263
        start_exact = [start_y * 100.0 / res - gx1, start_x * 100.0 / res - gy1]      # :264-266 (r = y, c = x)
        start = _threshold([int(start_y * 100.0 / res - gx1), int(start_x * 100.0 / res - gy1)], shape)
        # the previous position in THIS step's window (:272-277)
        last_x, last_y = self.last_loc[0], self.last_loc[1]
        last_start = _threshold([int(last_y * 100.0 / res - gx1), int(last_x * 100.0 / res - gy1)], shape)
        self.last_start = last_start
        cells = []
        if self.last_action == 1:                                                      # :283-320
            x1, y1, t1 = self.last_loc
            x2, y2, _ = self.curr_loc
            buf = 4 if self.prev_blocked < self.block_threshold else 2
            length = 2
            if abs(x1 - x2) < 0.05 and abs(y1 - y2) < 0.05:
                self.col_width += 2
                if self.col_width == 7:
                    length, buf = 4, 3
                self.col_width = min(self.col_width, 1)                                # (as written: the width never leaves 1, :294)
            else:
                self.col_width = 1
            dist = ((x1 - x2) ** 2 + (y1 - y2) ** 2) ** 0.5                            # pu.get_l2_distance (utils/pose.py:4-8)
            if dist < args.collision_threshold:
                self.prev_blocked += 1
                width = self.col_width
                full = tuple(int(v) for v in self.collision_map.shape)
                for i in range(length):
                    for j in range(width):
                        # the caller's NumPy owns the last bit of these (:304-312); the device gets integers
                        ahead, side = i + buf, j - width // 2
                        wx = x1 + 0.05 * (ahead * np.cos(np.deg2rad(t1)) + side * np.sin(np.deg2rad(t1)))
                        wy = y1 + 0.05 * (ahead * np.sin(np.deg2rad(t1)) - side * np.cos(np.deg2rad(t1)))
                        cells.append(tuple(_threshold([int(wy * 100 / res), int(wx * 100 / res)], full)))
            else:
                if self.prev_blocked >= self.block_threshold:
                    self.untrap.reset()
                self.prev_blocked = 0
        lmb = [gx1, gx2, gy1, gy2]
        return dict(start=start, start_exact=start_exact, start_o=start_o, lmb=lmb, cells=cells,
                    mark=(self.visited_vis, self.collision_map, lmb, last_start, start, cells))

    def _stg_inputs(self, planner_inputs, step):
        """The arguments of ``ShortTermGoal.get_stg`` for this step: the maps of ``planner_inputs`` where they lie (HIP tensors) or
        uploaded (NumPy), ``start_exact`` as ``_plan`` forms it (:264-266)."""
        dev = self.agent_states.device
        obstacle, goal = planner_inputs['obstacle'], planner_inputs['goal']
        if not isinstance(obstacle, torch.Tensor):
            obstacle = torch.as_tensor(np.ascontiguousarray(obstacle, dtype=np.float32)).to(dev)
        if not isinstance(goal, torch.Tensor):
            goal = torch.as_tensor(np.ascontiguousarray(np.asarray(goal) != 0).astype(np.uint8)).to(dev)
        return (obstacle, goal, self.collision_map, self.visited_vis, step['lmb'], [float(v) for v in step['start_exact']],
                planner_inputs['found_goal'], planner_inputs['goal_name'])

    def _get_stg(self, planner_inputs, step):
        """``_get_stg`` (:374-493) on the device -> ((stg_x, stg_y), stop); with ``only_explore`` a retry moves on to the next
        preset goal (:444-445)."""
        planner = self.agent_states._stg_planner()
        stg, stop = planner.get_stg(*self._stg_inputs(planner_inputs, step))
        return self._stg_done(planner, stg, stop)

    def _stg_done(self, planner, stg, stop):
        if planner.last['retried'] and self.args.only_explore:
            self.agent_states.next_preset_goal()
        self.agent_states.stg, self.agent_states.stg_stop = stg, stop
        return stg, stop

    def _plan_end(self, planner_inputs, step, stg, stop):
        """(:326-371) the action from the short-term goal: the stop countdown, the turn towards the goal, the untrap override."""
        self.stg = stg                                                                 # :492
        start, start_o = step['start'], step['start_o']
        if self.forward_after_stop < 0:                                                # :326-327
            self.forward_after_stop = self.forward_after_stop_preset
        if self.forward_after_stop != self.forward_after_stop_preset:                  # the countdown runs (:328-334)
            action = 0 if self.forward_after_stop == 0 else 1
            self.forward_after_stop -= 1
        elif stop and planner_inputs['found_goal'] == 1:                               # :335-340
            if self.forward_after_stop == 0:
                action = 0
            else:
                self.forward_after_stop -= 1
                action = 1
        else:
            stg_x, stg_y = stg
            stg_x = np.clip(stg_x, self.edge_buffer, self.local_w - self.edge_buffer - 1)      # stay inside the map (:345-346)
            stg_y = np.clip(stg_y, self.edge_buffer, self.local_h - self.edge_buffer - 1)
            angle_st_goal = math.degrees(math.atan2(stg_x - start[0], stg_y - start[1]))
            angle_agent = start_o % 360.0
            if angle_agent > 180:
                angle_agent -= 360
            relative_angle = (angle_agent - angle_st_goal) % 360.0
            if relative_angle > 180:
                relative_angle -= 360
            if relative_angle > self.args.turn_angle / 2.:
                action = 3
            elif relative_angle < -self.args.turn_angle / 2.:
                action = 2
            else:
                action = 1
        if self.prev_blocked >= self.block_threshold:                                  # :365-370
            action = self.untrap.get_action() if self._previous_action == 1 else 1
        self._previous_action = action
        return action


def plan_act_batch(helpers, planner_inputs, stg_batch=None):
    """``Agent_Helper.plan_act`` for the E episodes of a lock-step group -> E ``{'action': a}``: the E marks in ONE
    ``peanut_plan_mark_batch``, the E short-term goals in ONE ``planner.get_stg_batch``; every action, counter and map is what E
    single calls in this order give, bit for bit (the untrap's global RNG is drawn in episode order in both).  The helpers must
    share one device and one map shape.  ``stg_batch(helpers, planner_inputs, steps) -> E ((stg_x, stg_y), stop)`` replaces the
    device solve (tests)."""
    helpers, planner_inputs = list(helpers), list(planner_inputs)
    E = len(helpers)
    if E < 1 or E > _lib.PLAN_MAX_BATCH:
        raise ValueError(f"plan_act_batch takes 1..{_lib.PLAN_MAX_BATCH} episodes, got {E}")
    if len(planner_inputs) != E:
        raise ValueError(f"{len(planner_inputs)} planner inputs for {E} helpers")
    if len({id(h) for h in helpers}) != E or len({id(h.agent_states) for h in helpers}) != E:
        raise ValueError("the same helper or Agent_State appears twice")
    h0 = helpers[0]
    for e, h in enumerate(helpers):
        if h.visited_vis.shape != h0.visited_vis.shape or h.visited_vis.device != h0.visited_vis.device:
            raise ValueError(f"helper {e} differs from helper 0 in map shape or device: a mixed batch")
    for h, p in zip(helpers, planner_inputs):
        h.timestep += 1
        h.goal_name = p['goal_name']
    steps = [h._plan_begin(p) for h, p in zip(helpers, planner_inputs)]
    plan_mark_batch([s['mark'] for s in steps])
    if stg_batch is not None:
        stgs = list(stg_batch(helpers, planner_inputs, steps))
    elif E == 1:
        stgs = [h0._get_stg(planner_inputs[0], steps[0])]
    else:
        from .planner import get_stg_batch
        planners = [h.agent_states._stg_planner() for h in helpers]
        res = get_stg_batch(planners, [h._stg_inputs(p, s) for h, p, s in zip(helpers, planner_inputs, steps)])
        stgs = [h._stg_done(pl, stg, stop) for h, pl, (stg, stop) in zip(helpers, planners, res)]
    out = []
    for h, p, s, (stg, stop) in zip(helpers, planner_inputs, steps, stgs):
        action = h._plan_end(p, s, stg, stop)
        h.last_action = action
        out.append({'action': action})
    if getattr(h0.args, "visualize", 0):                             # the E frames in ONE render_batch and one read-back
        vis = h0._renderer()
        vis.render_batch([h.agent_states.vis_item(p, stg=h.stg, rgb=h.rgb_vis) for h, p in zip(helpers, planner_inputs)])
        for h, frame in zip(helpers, vis.frame_host()):
            h._keep_frame(frame)
    return out
