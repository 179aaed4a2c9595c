"""Device-resident counterpart of the hot-path CALLERS in the reference's ``Agent_State``
(nav/agent/agent_state.py): map/pose bookkeeping around ``Semantic_Mapping`` and
``PEANUT_Prediction_Model``.  Same attribute and method names, same call order, same arithmetic;
differences, all on purpose:

* ``full_map`` / ``local_map`` live on the HIP device for the whole episode and
  ``update_prediction`` crops, predicts, pads and masks ON the device (the reference copies the
  14x720x720 crop to the host, back to the GPU inside ``run_inference`` and the result back again,
  agent_state.py:361 -> prediction.py:128-131,268);
* long-term goal selection (``update_global_goal`` :376-415) runs on the device too (csrc/goal.hip: dilation,
  geodesic field, distance weights and the argmax; scikit-fmm's fast marching replaced by a fixed-point solver of
  the same discretisation).  ``collision_map`` / ``visited_vis``, which the reference
  reads from ``self.helper`` (the CPU planner's bookkeeping), are attributes here (uint8 HIP tensors, zero until
  ``Agent_Helper`` writes them);
* ``update_goal_map`` (:418-446: whether the goal category is in the local map, after ``goal_erode`` erosions, a dilation and
  the "no other category claims the cell" mask) and the planner-input dict (:251-257) are here behind ``args.goal_map`` (a
  peanut_amd-only switch, default off): two launches on the local map where it lies (csrc/goal_map.hip) and a 4-byte read-back
  instead of a device reduction, a copy of the plane to the host and up to four scikit-image passes there.  ``planner_inputs``
  is what the reference's ``Agent_Helper.plan_act`` takes;
* of the local planner, ``_get_stg`` (agent_helper.py:374-493) is here as ``short_term_goal`` behind ``args.plan_stg`` (default
  off, needs ``args.goal_map``; csrc/stg.hip through ``peanut_amd.planner.ShortTermGoal``); the scalar state machine around it
  (``_plan``: collision and visited bookkeeping, action choice, untrap) is ``peanut_amd.agent_helper.Agent_Helper``, on the host
  as in the reference; it writes ``collision_map`` / ``visited_vis`` in place with one launch per step (csrc/plan.hip) and is
  reached through ``args.plan_act`` (``PEANUT_Agent``) or ``Agent_State_Group.plan_acts``.

The 12-byte pose read-back per step (`local_pose.cpu()`, :276) is kept: the integer cell indices it
yields drive the host-side decisions exactly as in the reference.  The eight small tensor operations that follow it
(:281-296: clear the location channel, trajectory square, explored-area footprints) are one launch
(``peanut_map_mark_agent``), and the sensor pose goes up through a pinned staging buffer."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .mapping import Semantic_Mapping
from .prediction import PEANUT_Prediction_Model


def default_args(**over):
    """The flags of nav/arguments.py the hot-path callers read, at their defaults (``argparse.Namespace``), for
    drivers that run without the reference's argument parser (tools/bench_pipeline.py)."""
    from argparse import Namespace
    a = dict(seed=1, cuda=False, sem_gpu_id=0, num_sem_categories=10, map_size_cm=4800, map_resolution=5,
             global_downscaling=2, only_explore=1, col_rad=4, grid_resolution=24, num_local_steps=20,
             switch_step=0, update_goal_freq=10, goal_reached_dist=75, prediction_window=720, visualize=0,
             frame_height=120, frame_width=160, env_frame_height=480, env_frame_width=640, vision_range=100,
             hfov=79.0, du_scale=1, cat_pred_threshold=5.0, exp_pred_threshold=1.0, map_pred_threshold=0.1,
             camera_height=0.88, min_depth=0.5, max_depth=5.0, sem_pred_prob_thr=0.95, goal_thr=0.985,
             dist_weight_temperature=500, timestep_limit=499, goal_map=False, goal_erode=3, plan_stg=False,
             magnify_goal_when_hard=100, plan_act=False, turn_angle=30, collision_threshold=0.20, move_forward_after_stop=1)
    a.update(over)
    return Namespace(**a)


def disk(radius, dtype=np.uint8):
    """``skimage.morphology.disk`` (all pixels with x^2 + y^2 <= r^2); scikit-image is only needed
    for this footprint (agent_state.py:85-86)."""
    L = np.arange(-radius, radius + 1)
    X, Y = np.meshgrid(L, L)
    return np.array((X ** 2 + Y ** 2) <= radius ** 2, dtype=dtype)


class Agent_State:
    """Hot-path subset of ``Agent_State`` (agent_state.py:26-454)."""

    def __init__(self, args, prediction_model=None, state_dict=None):
        self.args = args
        self.device = args.device = torch.device("cuda:" + str(args.sem_gpu_id))
        self.nc = 4 + args.num_sem_categories
        self.map_size = args.map_size_cm // args.map_resolution
        self.full_w, self.full_h = self.map_size, self.map_size
        self.local_w = int(self.full_w / args.global_downscaling)
        self.local_h = int(self.full_h / args.global_downscaling)
        self.full_map = torch.zeros(self.nc, self.full_w, self.full_h, dtype=torch.float32, device=self.device)
        self.local_map = torch.zeros(self.nc, self.local_w, self.local_h, dtype=torch.float32, device=self.device)
        self.full_pose = torch.zeros(3, dtype=torch.float32, device=self.device)
        self.local_pose = torch.zeros(3, dtype=torch.float32, device=self.device)
        self.origins = np.zeros((3))
        self.lmb = np.zeros((4)).astype(int)
        self.planner_pose_inputs = np.zeros((7))
        self.sem_map_module = Semantic_Mapping(args).to(self.device)
        self.sem_map_module.eval()
        # preset corner goals of the exploration policy (agent_state.py:79-80); inert at the default switch_step = 0
        self.global_goal_presets = [(0.1, 0.1), (0.9, 0.1), (0.9, 0.9), (0.1, 0.9)]
        self.global_goal_preset_id = 0
        self.helper = None                      # the Agent_Helper that plans for this state, once one is made
        if prediction_model is not None:
            self.prediction_model = prediction_model
        elif getattr(args, "only_explore", 0) == 0:
            self.prediction_model = PEANUT_Prediction_Model(args, state_dict=state_dict)
        else:
            self.prediction_model = None
        self.selem = disk(args.col_rad)
        sel = np.where(disk(args.col_rad + 1) > 0)
        self.selem_idx = sel
        self._selem_r = torch.from_numpy(sel[0].astype(np.int64)).to(self.device)
        self._selem_c = torch.from_numpy(sel[1].astype(np.int64)).to(self.device)
        self._selem_mask = torch.from_numpy(np.ascontiguousarray(disk(args.col_rad + 1))).to(self.device)     # uint8 [(2R+1)^2]
        self._pose_host = torch.zeros(3, dtype=torch.float32).pin_memory()      # staging of the per-step sensor pose
        self.target_pred = None
        # what only the visualisation frame reads (agent_state.py:87-88, :409-410), kept with args.visualize: views into the goal solver
        self.dd_wt = None
        self.value = None
        if getattr(args, "visualize", 0) and float(getattr(args, "dist_weight_temperature", 500)) == 0:
            raise NotImplementedError("args.visualize with dist_weight_temperature == 0: the goal solver keeps no distance weights in "
                                      "frontier mode, so the frame's two right panels have no source")
        self.global_goals = [[0, 0]]
        self.dist_to_goal = float("inf")
        # long-term goal selection (agent_state.py:376-415); the planner-side maps live here as HIP tensors
        self.collision_map = torch.zeros((self.full_w, self.full_h), dtype=torch.uint8, device=self.device)
        self.visited_vis = torch.zeros((self.full_w, self.full_h), dtype=torch.uint8, device=self.device)
        self._goal = None
        self.last_global_goal = None
        self.value_max = None
        # update_goal_map (agent_state.py:418-446): the goal map stays on the device, found_goal comes back through a pinned word
        self.goal_map = None
        self.found_goal = False
        self._found_dev = None
        self._found_host = None
        # the local planner's short-term goal (agent_helper.py:374-493), behind args.plan_stg
        self._stg = None
        self.stg = None
        self.stg_stop = None

    # ---- agent_state.py:94-105 ----
    def reset(self):
        self.l_step = 0
        self.step = 0
        self.goal_cat = -1
        self.found_goal = False
        self.goal_map = None
        self.init_map_and_pose()
        self.target_pred = None
        self.dd_wt = None                       # (agent_state.py:99-101)
        self.value = None
        self.last_global_goal = None
        self.collision_map.zero_()              # Agent_Helper.reset (agent_helper.py:114-115)
        self.visited_vis.zero_()
        if self._goal is not None:
            self._goal.reset()                  # self.dd_wt = None

    # ---- agent_state.py:154-178 ----
    def get_local_map_boundaries(self, agent_loc, local_sizes, full_sizes):
        loc_r, loc_c = agent_loc
        local_w, local_h = local_sizes
        full_w, full_h = full_sizes
        if self.args.global_downscaling > 1:
            gx1, gy1 = loc_r - local_w // 2, loc_c - local_h // 2
            gx1, gy1 = gx1 - gx1 % self.args.grid_resolution, gy1 - gy1 % self.args.grid_resolution
            gx2, gy2 = gx1 + local_w, gy1 + local_h
            if gx1 < 0:
                gx1, gx2 = 0, local_w
            if gx2 > full_w:
                gx1, gx2 = full_w - local_w, full_w
            if gy1 < 0:
                gy1, gy2 = 0, local_h
            if gy2 > full_h:
                gy1, gy2 = full_h - local_h, full_h
        else:
            gx1, gx2, gy1, gy2 = 0, full_w, 0, full_h
        return [gx1, gx2, gy1, gy2]

    def _rebind_local(self):
        """lmb / origins / local view / local pose from the full pose (shared tail of
        init_map_and_pose :197-210 and update_full_map :318-331)."""
        args = self.args
        locs = self.full_pose.cpu().numpy()
        r, c = locs[1], locs[0]
        loc_r, loc_c = [int(r * 100.0 / args.map_resolution), int(c * 100.0 / args.map_resolution)]
        self.lmb = self.get_local_map_boundaries((loc_r, loc_c), (self.local_w, self.local_h),
                                                 (self.full_w, self.full_h))
        self.planner_pose_inputs[3:] = self.lmb
        self.origins = np.array([self.lmb[2] * args.map_resolution / 100.0,
                                 self.lmb[0] * args.map_resolution / 100.0, 0.])
        self.local_map = self.full_map[:, self.lmb[0]:self.lmb[1], self.lmb[2]:self.lmb[3]]
        self.local_pose = self.full_pose - torch.from_numpy(self.origins).to(self.device).float()
        return locs, loc_r, loc_c

    # ---- agent_state.py:181-210 ----
    def init_map_and_pose(self):
        args = self.args
        self.full_map.fill_(0.)
        self.full_pose.fill_(0.)
        self.full_pose[:2] = self.args.map_size_cm / 100.0 / 2.0
        locs = self.full_pose.cpu().numpy()
        self.planner_pose_inputs[:3] = locs
        r, c = locs[1], locs[0]
        loc_r, loc_c = [int(r * 100.0 / args.map_resolution), int(c * 100.0 / args.map_resolution)]
        self.full_map[2:4, loc_r - 1:loc_r + 2, loc_c - 1:loc_c + 2] = 1.0
        self._rebind_local()

    def _map_step(self, obs):
        """``_, self.local_map, _, self.local_pose = self.sem_map_module(obs, self.poses,
        self.local_map, self.local_pose, self)`` (:114-115, :273-274).  The HIP module needs contiguous
        inputs; a view into full_map is copied first, like the reference's `maps_last[None,:]` cat."""
        lm = self.local_map if self.local_map.is_contiguous() else self.local_map.contiguous()
        lp = self.local_pose if self.local_pose.is_contiguous() else self.local_pose.contiguous()
        _, self.local_map, _, self.local_pose = self.sem_map_module(obs, self.poses, lm, lp, self)

    # ---- agent_state.py:108-150 (map part) ----
    def init_with_obs(self, obs, infos):
        self.l_step = 0
        self.step = 0
        self.poses = torch.from_numpy(np.asarray(infos['sensor_pose'])).float().to(self.device)
        self._map_step(obs)
        self.locs = self.local_pose.cpu().numpy()
        r, c = self.locs[1], self.locs[0]
        loc_r, loc_c = [int(r * 100.0 / self.args.map_resolution), int(c * 100.0 / self.args.map_resolution)]
        self.local_map[2:4, loc_r - 1:loc_r + 2, loc_c - 1:loc_c + 2] = 1.
        rgoal = [0.1, 0.1]
        self.global_goals = [[int(rgoal[0] * self.local_w), int(rgoal[1] * self.local_h)]]
        self.global_goals = [[min(x, int(self.local_w - 1)), min(y, int(self.local_h - 1))]
                             for x, y in self.global_goals]

    # ---- agent_state.py:268-300 ----
    def update_local_map(self, obs):
        self._map_step(obs)
        locs = self.local_pose.cpu().numpy()
        loc_r, loc_c, traj_rad, centres = self._local_map_host(locs)
        self._mark_agent(loc_r, loc_c, traj_rad, centres)
        self.loc_r = loc_r
        self.loc_c = loc_c

    def _local_map_host(self, locs):
        """The host decisions of ``update_local_map`` (:276-291) from the pose that was read back: planner pose, agent cell,
        distance to the goal, and what to mark -- (loc_r, loc_c, traj_rad, centres) for ``_mark_agent``.  Shared by the
        single-episode step above and ``Agent_State_Group``, which reads the poses of all its episodes back at once."""
        args = self.args
        self.planner_pose_inputs[:3] = locs + self.origins
        r, c = locs[1], locs[0]
        loc_r = int(r * 100.0 / args.map_resolution)
        loc_c = int(c * 100.0 / args.map_resolution)
        traj_rad = 2
        self.dist_to_goal = np.sqrt((loc_r - (self.global_goals[0][0])) ** 2 +
                                    (loc_c - (self.global_goals[0][1])) ** 2) * args.map_resolution
        centres = [(loc_r, loc_c)]
        if self.dist_to_goal < args.goal_reached_dist:
            centres.append((self.global_goals[0][0], self.global_goals[0][1]))
        return loc_r, loc_c, traj_rad, centres

    def _upload_pose(self, sensor_pose):
        """``torch.from_numpy(np.asarray(infos['sensor_pose'])).float().to(device)`` (:225) through one pinned buffer: the copy is
        asynchronous, and the buffer is free again by the next step because update_local_map reads the pose back (a device
        synchronisation) after the projection that consumes it."""
        self._pose_host.copy_(torch.from_numpy(np.asarray(sensor_pose, dtype=np.float64)).float())
        return self._pose_host.to(self.device, non_blocking=True)

    def _mark_agent(self, loc_r, loc_c, traj_rad, centres):
        """(:281-296) in one launch (``peanut_map_mark_agent``)::

            self.local_map[2, :, :].fill_(0.)
            self.local_map[2:4, loc_r - traj_rad:loc_r + traj_rad + 1, loc_c - traj_rad:loc_c + traj_rad + 1] = 1.
            self.local_map[1][self.selem_idx[0] - int(args.col_rad + 1) + r, self.selem_idx[1] - int(args.col_rad + 1) + c] = 1.
                                                                   # for (r, c) in centres: the agent, and the goal once reached

        with Python's slice clamping and torch's index rules (negative wraps, out of range raises IndexError)."""
        lm, m, rad, (r0, r1, c0, c1) = self._mark_args(loc_r, loc_c, traj_rad, centres)
        flat = (C.c_int * (2 * len(centres)))(*[int(v) for rc in centres for v in rc])
        with torch.cuda.device(self.device):
            rc = _lib.load().peanut_map_mark_agent(lm.data_ptr(), int(lm.shape[0]), m, r0, r1, c0, c1, self._selem_mask.data_ptr(), rad,
                                                   len(centres), C.byref(flat), _lib.current_stream_ptr(self.device))
        _lib.check(rc, "peanut_map_mark_agent")

    def _mark_args(self, loc_r, loc_c, traj_rad, centres):
        """The checks of ``_mark_agent`` and the normalised trajectory square: (local_map, m, footprint radius, (r0, r1, c0, c1))."""
        lm = self.local_map
        if not lm.is_contiguous():            # (a view into full_map right after _rebind_local; _map_step replaces it)
            raise RuntimeError("local_map must be contiguous here")
        if lm.dtype != torch.float32 or lm.shape[1] != lm.shape[2]:
            # peanut_map_mark_agent takes ONE side length (row / column decomposition, plane stride, index checks) and fp32 planes:
            # the reference's local map is square (agent_state.py:56-60: local_w = local_h); anything else is refused, not mis-indexed
            raise ValueError(f"_mark_agent: the local map must be a square fp32 [C, M, M] tensor, got {tuple(lm.shape)} {lm.dtype}")
        m = int(lm.shape[1])
        rad = int(self.args.col_rad + 1)
        r0, r1, _ = slice(loc_r - traj_rad, loc_r + traj_rad + 1).indices(m)
        c0, c1, _ = slice(loc_c - traj_rad, loc_c + traj_rad + 1).indices(int(lm.shape[2]))
        for cr, cc in centres:
            if cr - rad < -m or cr + rad >= m or cc - rad < -m or cc + rad >= m:
                raise IndexError(f"explored-area footprint around ({cr}, {cc}) leaves the {m} x {m} local map")
        return lm, m, rad, (r0, r1, c0, c1)

    # ---- agent_state.py:303-338 ----
    def update_full_map(self):
        args = self.args
        self.full_map[:, self.lmb[0]:self.lmb[1], self.lmb[2]:self.lmb[3]] = self.local_map
        self.full_pose = self.local_pose + torch.from_numpy(self.origins).to(self.device).float()
        self._rebind_local()
        locs = self.local_pose.cpu().numpy()
        r, c = locs[1], locs[0]
        self.loc_r = int(r * 100.0 / args.map_resolution)
        self.loc_c = int(c * 100.0 / args.map_resolution)

    # ---- agent_state.py:345-373, on the device ----
    def update_prediction(self, goal_follows=False):
        crop = self._prediction_input(goal_follows)
        self._prediction_output(self.prediction_model.get_prediction_batch(crop)[0])

    def _prediction_input(self, goal_follows=False):
        """First half of ``update_prediction``: the local map written back, the goal solver begun, and the [1,C,W,W] window the
        prediction model reads (the whole full map, or its centre crop)."""
        args = self.args
        self.full_map[:, self.lmb[0]:self.lmb[1], self.lmb[2]:self.lmb[3]] = self.local_map
        if goal_follows and getattr(args, "goal_overlap", True):
            # update_global_goal follows at once (update_state, :240-245): its geodesic field needs the map as it is NOW, not
            # the prediction -- begun here, the solver runs it on its own stream beside the forward below (include/peanut_hip.h)
            self._goal_solver().select_begin(self.full_map[0], self.collision_map, self.visited_vis, self.lmb, (self.loc_r, self.loc_c))
        return self._prediction_crop()

    def _prediction_crop(self):
        """The [1,C,W,W] window of the full map the prediction model reads."""
        args = self.args
        if self.full_w == args.prediction_window and self.full_h == args.prediction_window:
            return self.full_map[None].contiguous()
        x1 = self.full_w // 2 - args.prediction_window // 2
        x2 = x1 + args.prediction_window
        y1 = self.full_h // 2 - args.prediction_window // 2
        y2 = y1 + args.prediction_window
        return self.full_map[:, x1:x2, y1:y2].contiguous()[None]

    def _prediction_output(self, preds):
        """Second half of ``update_prediction``: ``preds`` [K,W,W] of this episode's window -> ``target_pred``."""
        args = self.args
        if self.full_w == args.prediction_window and self.full_h == args.prediction_window:
            object_preds = preds
        else:
            x1 = self.full_w // 2 - args.prediction_window // 2
            x2 = x1 + args.prediction_window
            y1 = self.full_h // 2 - args.prediction_window // 2
            y2 = y1 + args.prediction_window
            object_preds = torch.zeros((preds.shape[0], self.full_w, self.full_h), dtype=preds.dtype,
                                       device=preds.device)
            object_preds[:, x1:x2, y1:y2] = preds
        target = self.goal_cat
        target_pred = object_preds[target, self.lmb[0]:self.lmb[1], self.lmb[2]:self.lmb[3]]
        target_pred = target_pred * (self.local_map[1] < 0.5)        # unexplored regions only
        self.target_pred = target_pred

    def _goal_solver(self):
        if self._goal is None:
            from .goal import GeodesicSolver
            self._goal = GeodesicSolver(self.full_w, self.full_h, int(self.args.col_rad), device=self.device)
        return self._goal

    # ---- agent_state.py:376-415, on the device ----
    def update_global_goal(self):
        """Geodesic-distance-weighted argmax of the target prediction (csrc/goal.hip).  Needs ``target_pred`` (from
        ``update_prediction``) unless ``dist_weight_temperature == 0``."""
        args = self.args
        res = self._goal_solver().select(*self._goal_inputs(), self.target_pred, float(getattr(args, "dist_weight_temperature", 500)),
                                         int(args.map_resolution))
        self._goal_result(res)

    def _goal_inputs(self):
        """What the goal solver reads of this episode: (full_obstacle, collision_map, visited_vis, lmb, loc_rc)."""
        return self.full_map[0], self.collision_map, self.visited_vis, self.lmb, (self.loc_r, self.loc_c)

    def _goal_result(self, res):
        """The host bookkeeping of ``update_global_goal`` (:410-415) from one ``select`` / ``select_batch`` result."""
        self.value_max = res["value_max"]
        if getattr(self.args, "visualize", 0):            # self.dd_wt / self.value (:409-410) where the solver left them: no copy
            self.dd_wt, self.value = self._goal_solver().fields()
        self.goal_rounds = res["rounds"]
        self.goal_passes, self.goal_converged = res["passes"], res["converged"]
        new_global_goal = [res["goal"]]
        if new_global_goal != self.last_global_goal:      # avoid repeating the last goal
            self.last_global_goal = self.global_goals
            self.global_goals = new_global_goal

    # ---- agent_state.py:418-446, on the device ----
    def update_goal_map(self, infos):
        """``goal_map`` (uint8 HIP tensor [local_w, local_h], the same buffer on every step) and ``found_goal`` (0 / 1) from the
        local map where it lies -- contiguous or a view into the full map -- in two launches (``peanut_goal_map``) and one 4-byte
        read-back.  ``local_map`` is only read."""
        lm, ps, rs, params = self._goal_map_args(infos)
        if self._found_dev is None:
            self._found_dev = torch.zeros(1, dtype=torch.int32, device=self.device)
            self._found_host = torch.zeros(1, dtype=torch.int32).pin_memory()
        with torch.cuda.device(self.device):
            rc = _lib.load().peanut_goal_map(lm.data_ptr(), int(lm.shape[0]), int(lm.shape[1]), ps, rs, *params, self.goal_map.data_ptr(),
                                             self._found_dev.data_ptr(), _lib.current_stream_ptr(self.device))
            _lib.check(rc, "peanut_goal_map")
            self._found_host.copy_(self._found_dev, non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()
        self.found_goal = int(self._found_host[0])

    def _goal_map_args(self, infos):
        """What ``peanut_goal_map`` reads of this episode: (local_map, plane stride, row stride, (cn, morph, n_erode, detect, goal_r,
        goal_c)); allocates ``goal_map`` on first use.  :428-429 (only_explore, cn), :437-438 (no erosion for a tv: too thin)."""
        args = self.args
        lm = self.local_map
        if lm.dtype != torch.float32 or lm.dim() != 3 or lm.shape[1] != lm.shape[2] or lm.stride(2) != 1:
            raise ValueError(f"update_goal_map: the local map must be a square fp32 [C, M, M] tensor with unit column stride, got "
                             f"{tuple(lm.shape)} {lm.dtype} strides {tuple(lm.stride())}")
        if self.goal_map is None:
            self.goal_map = torch.empty((self.local_w, self.local_h), dtype=torch.uint8, device=self.device)
        params = (int(self.goal_cat) + 4, int('tv' not in infos.get('goal_name', '')), int(getattr(args, 'goal_erode', 3)),
                  int(args.only_explore == 0), int(self.global_goals[0][0]), int(self.global_goals[0][1]))
        return lm, int(lm.stride(0)), int(lm.stride(1)), params

    # ---- agent_state.py:251-257 ----
    def planner_inputs(self, infos, host=True):
        """The dict ``update_state`` hands to ``Agent_Helper.plan_act`` in the reference.  ``host=True``: NumPy with the
        reference's dtypes and shapes (obstacle / exp_pred float32 copies, goal float64 0/1, pose_pred a copy); ``host=False``: the
        same keys as HIP tensors / views, nothing copied.  ``sem_map_pred`` (:259-262) is there only with ``args.visualize``:
        int64 NumPy from one arg-max launch (``peanut_vis_sem_argmax``) with ``host=True``; with ``host=False`` the local map itself,
        the source the device renderer takes the arg-max from inside its own first launch."""
        if self.goal_map is None:
            raise RuntimeError("planner_inputs needs update_goal_map (args.goal_map) to have run on this step")
        visualize = bool(getattr(self.args, "visualize", 0))
        if not host:
            p = {'obstacle': self.local_map[0], 'exp_pred': self.local_map[1], 'pose_pred': self.planner_pose_inputs,
                 'goal': self.goal_map, 'found_goal': self.found_goal, 'goal_name': infos['goal_name']}
            if visualize:
                p['sem_map_pred'] = self.local_map
            return p
        p = {'obstacle': np.ascontiguousarray(self.local_map[0].cpu().numpy()),
             'exp_pred': np.ascontiguousarray(self.local_map[1].cpu().numpy()),
             'pose_pred': self.planner_pose_inputs.copy(),
             'goal': self.goal_map.cpu().numpy().astype(np.float64),
             'found_goal': self.found_goal, 'goal_name': infos['goal_name']}
        if visualize:
            from .vis import sem_argmax
            p['sem_map_pred'] = sem_argmax(self.local_map).cpu().numpy().astype(np.int64)
        return p

    def vis_item(self, planner_inputs, stg=None, rgb=None):
        """What ``vis.VisRenderer.render`` takes of this episode on this step (``Agent_Helper._visualize``)."""
        args = self.args
        gx1, gx2, gy1, gy2 = (int(v) for v in planner_inputs['pose_pred'][3:7])
        whole = self.full_w == args.prediction_window and self.full_h == args.prediction_window
        return dict(local_map=self.local_map, collision_map=self.collision_map, visited_vis=self.visited_vis, lmb=[gx1, gx2, gy1, gy2],
                    goal=planner_inputs['goal'], stg=stg, pose_pred=np.asarray(planner_inputs['pose_pred'], np.float64),
                    goal_name=planner_inputs['goal_name'], rgb=rgb, target_pred=self.target_pred, value=self.value, dd_wt=self.dd_wt,
                    target_bits=32 if whole else 64)                    # (:362: a float64 `temp` unless the window is the whole map)

    # ---- agent_helper.py:256-266 + 374-493, on the device ----
    def short_term_goal(self, infos):
        """What ``Agent_Helper._plan`` gets from ``_get_stg`` on this step's planner inputs: ((stg_x, stg_y), stop), from
        ``local_map[0]``, ``goal_map``, ``collision_map``, ``visited_vis``, ``lmb`` and the pose where they lie on the device
        (``peanut_stg_plan``); ``start_exact`` as ``_plan`` forms it (:264-266).  Needs ``update_goal_map`` to have run on this
        step.  The whole result stays in ``self._stg.last``."""
        if not getattr(self.args, "plan_stg", False):
            raise RuntimeError("short_term_goal is behind args.plan_stg (default off)")
        if self.goal_map is None:
            raise RuntimeError("short_term_goal needs update_goal_map (args.goal_map) to have run on this step")
        self.stg, self.stg_stop = self._stg_planner().get_stg(*self._stg_inputs(infos))
        return self.stg, self.stg_stop

    def _stg_planner(self):
        if self._stg is None:
            from .planner import ShortTermGoal
            self._stg = ShortTermGoal(self.args, device=self.device)
        return self._stg

    def _stg_inputs(self, infos):
        """The arguments of ``ShortTermGoal.get_stg`` on this step; ``start_exact`` as ``_plan`` forms it (:264-266)."""
        args = self.args
        start_x, start_y, _, gx1, gx2, gy1, gy2 = self.planner_pose_inputs
        lmb = [int(gx1), int(gx2), int(gy1), int(gy2)]
        r, c = start_y, start_x
        start_exact = [r * 100.0 / args.map_resolution - lmb[0], c * 100.0 / args.map_resolution - lmb[2]]
        return (self.local_map[0], self.goal_map, self.collision_map, self.visited_vis, lmb, start_exact, self.found_goal,
                infos['goal_name'])

    # ---- agent_state.py:341-342 ----
    def next_preset_goal(self):
        self.global_goal_preset_id = (self.global_goal_preset_id + 1) % len(self.global_goal_presets)

    # ---- agent_state.py:449-454 ----
    def inc_step(self):
        args = self.args
        self.l_step += 1
        self.step += 1
        self.l_step = self.step % args.num_local_steps

    # ---- perception half of update_state (agent_state.py:213-245) ----
    def update_state(self, obs, infos):
        """Map update -> (every num_local_steps) full-map update -> (every update_goal_freq steps,
        at step 0, or near the goal) prediction + long-term goal selection (:240-245; ``args.select_goal = False``
        skips the latter), then with ``args.goal_map`` on ``update_goal_map`` (:247).  Returns whether a prediction ran; the
        planner-input dict (:251-257) is ``planner_inputs(infos)``."""
        args = self.args
        self.goal_cat = infos['goal_cat_id']
        self.poses = self._upload_pose(infos['sensor_pose'])
        self.update_local_map(obs)
        self._step_full_map()
        predicted = False
        if self._prediction_due():
            select = getattr(args, "select_goal", True)
            self.update_prediction(goal_follows=select)
            if select:
                self.update_global_goal()
            predicted = True
        if getattr(args, "goal_map", False):
            self.update_goal_map(infos)
        self.inc_step()
        return predicted

    def _step_full_map(self):
        """(:231-235) the local period: every ``num_local_steps`` steps the local map goes back into the full map."""
        if self.l_step == self.args.num_local_steps - 1:
            self.l_step = 0
            self.update_full_map()
            if self.step < self.args.switch_step:           # no prediction yet: head for a preset corner (:231-237)
                preset = self.global_goal_presets[self.global_goal_preset_id]
                self.global_goals = [[int(preset[0] * self.local_w), int(preset[1] * self.local_h)]]
                self.global_goals = [[min(x, int(self.local_w - 1)), min(y, int(self.local_h - 1))] for x, y in self.global_goals]

    def _prediction_due(self):
        """(:240) whether this step predicts and selects a goal."""
        args = self.args
        return (self.step % args.update_goal_freq == args.update_goal_freq - 1 or self.step == 0 or
                self.dist_to_goal < args.goal_reached_dist) and self.step >= args.switch_step \
            and self.prediction_model is not None


class Agent_State_Group:
    """E ``Agent_State`` objects on one device stepped in lock-step, so that the map projection sees a batch of E: the
    one-process counterpart of the reference's several environments per GPU (nav/collect.py:32-50, ``--sem_gpu_id``).

    Per step: one pinned ``[E,3]`` pose upload, one ``Semantic_Mapping.forward_batch``, ONE ``[E,3]`` pose read-back, the host
    decisions of ``update_local_map`` per episode, one ``peanut_map_mark_agent_batch``, then per episode exactly what
    ``Agent_State.update_state`` does afterwards.  Every episode ends a step with the bits it would have stepping alone.
    ``batch_predictions=True`` runs the episodes that predict on the same step through one ``get_prediction_batch`` call; a
    batched forward differs from batch 1 in the last fp32 bits, hence opt-in.  ``batch_goals`` (default on): when at least two
    episodes predict on a step with ``select_goal`` on, their long-term goals are selected in ONE batched solve
    (``goal.select_batch``: the launches and synchronisations of one solve instead of E in a row), begun for all of them before
    their prediction forwards; every episode's field, weights and goal are the bits of its own ``update_global_goal``.
    With ``args.goal_map`` on, the goal maps of all active episodes of a step go through ONE ``peanut_goal_map_batch`` call and ONE
    ``[E]`` read-back, after every episode's goal of that step is final and before any ``inc_step``.
    ``short_term_goals`` (``batch_stg``, default on) is ``short_term_goal`` for the active episodes in ONE ``get_stg_batch`` per group
    of planner shapes: the solves and synchronisations of the longest chain among the episodes instead of all chains in a row.

    The states share one ``Semantic_Mapping`` handle, reserved for ``max_batch`` episodes (default: all of them).  The batch
    is ``self.active``, in order; ``drop`` takes an episode out (it ended), ``reset_active`` puts all back."""

    MAP_FIELDS = ("frame_height", "frame_width", "map_resolution", "map_size_cm", "global_downscaling", "vision_range", "hfov",
                  "du_scale", "cat_pred_threshold", "exp_pred_threshold", "map_pred_threshold", "num_sem_categories",
                  "camera_height", "col_rad")

    def __init__(self, states, max_batch=None, batch_predictions=False, batch_goals=True, batch_stg=True):
        states = list(states)
        if not states:
            raise ValueError("Agent_State_Group needs at least one state")
        max_batch = len(states) if max_batch is None else int(max_batch)
        if not 1 <= max_batch <= Semantic_Mapping.MAX_BATCH:
            raise ValueError(f"max_batch must be 1..{Semantic_Mapping.MAX_BATCH}, got {max_batch}")
        if len(states) > max_batch:
            raise ValueError(f"{len(states)} episodes exceed the reserve of {max_batch}")
        if len({id(s) for s in states}) != len(states):
            raise ValueError("the same Agent_State appears twice")
        first = states[0]
        for e, s in enumerate(states[1:], 1):
            if s.device != first.device:
                raise ValueError(f"state {e} lives on {s.device}, state 0 on {first.device}")
            diff = [f for f in self.MAP_FIELDS if getattr(s.args, f) != getattr(first.args, f)]
            if diff:
                raise ValueError(f"state {e} differs from state 0 in the mapping arguments {diff}")
        self.states = states
        self.active = list(states)
        self.device = first.device
        self.batch_predictions = bool(batch_predictions)
        self.batch_goals = bool(batch_goals)
        self.goal_batches = 0              # select_batch calls so far (diagnostics)
        self.goal_map_batches = 0          # peanut_goal_map_batch calls so far (diagnostics)
        self.batch_stg = bool(batch_stg)
        self.stg_batches = 0               # get_stg_batch calls so far (diagnostics)
        self.plan_batches = 0              # plan_act_batch calls so far (diagnostics)
        self._found_dev = None
        self._found_host = None
        self.sem_map_module = first.sem_map_module
        self.sem_map_module.reserve(max_batch)
        for s in states:
            s.sem_map_module = self.sem_map_module
        self.max_batch = max_batch
        self._poses_host = self._pinned(max_batch)

    # ---- the device calls (everything else in this class is host logic) ----
    @staticmethod
    def _pinned(n):
        return torch.zeros((n, 3), dtype=torch.float32).pin_memory()

    def _upload_poses(self, sensor_poses):
        """E sensor poses through one pinned buffer, one asynchronous copy (``Agent_State._upload_pose`` for the batch)."""
        E = len(sensor_poses)
        self._poses_host[:E].copy_(torch.from_numpy(np.asarray(sensor_poses, dtype=np.float64).reshape(E, 3)).float())
        return self._poses_host[:E].to(self.device, non_blocking=True)

    def _map_step(self, obs, poses):
        """One ``forward_batch`` over the active episodes; the one pose read-back of the step.  Returns locs [E,3] (host)."""
        act = self.active
        maps_last = [s.local_map if s.local_map.is_contiguous() else s.local_map.contiguous() for s in act]
        local_poses = torch.stack([s.local_pose for s in act])
        _, map_pred, _, local_poses = self.sem_map_module.forward_batch(obs, poses, maps_last, local_poses)
        for e, s in enumerate(act):
            s.poses = poses[e]
            s.local_map = map_pred[e]
            s.local_pose = local_poses[e]
        return local_poses.cpu().numpy()

    def _mark_agent_batch(self, marks):
        """``marks``: per active episode (local_map, m, footprint radius, (r0, r1, c0, c1), centres) -> one launch."""
        E = len(marks)
        lm0, m, rad = marks[0][0], marks[0][1], marks[0][2]
        maps = (C.c_void_p * E)(*[mk[0].data_ptr() for mk in marks])
        squares = (C.c_int * (4 * E))(*[int(v) for mk in marks for v in mk[3]])
        n_centres = (C.c_int * E)(*[len(mk[4]) for mk in marks])
        flat = [0] * (4 * E)
        for e, mk in enumerate(marks):
            for k, (cr, cc) in enumerate(mk[4]):
                flat[4 * e + 2 * k], flat[4 * e + 2 * k + 1] = int(cr), int(cc)
        centres = (C.c_int * (4 * E))(*flat)
        with torch.cuda.device(self.device):
            rc = _lib.load().peanut_map_mark_agent_batch(E, maps, int(lm0.shape[0]), m, squares, self.active[0]._selem_mask.data_ptr(),
                                                         rad, n_centres, centres, _lib.current_stream_ptr(self.device))
        _lib.check(rc, "peanut_map_mark_agent_batch")

    def _goal_begin_batch(self, states):
        """One ``select_begin_batch`` for these episodes (their full maps are final here)."""
        from .goal import select_begin_batch
        select_begin_batch([s._goal_solver() for s in states], [s._goal_inputs() for s in states])

    def _goal_select_batch(self, states):
        """One ``select_batch`` for these episodes -> their E result dicts."""
        from .goal import select_batch
        args = states[0].args
        return select_batch([s._goal_solver() for s in states], [s._goal_inputs() for s in states], [s.target_pred for s in states],
                            float(getattr(args, "dist_weight_temperature", 500)), int(args.map_resolution))

    def _goal_map_batch(self, maps):
        """``maps``: per episode what ``Agent_State._goal_map_args`` returns plus its goal_map tensor -> one call, one read-back.
        Returns the E found flags."""
        E = len(maps)
        lm0 = maps[0][0]
        if self._found_dev is None:
            self._found_dev = torch.zeros(self.max_batch, dtype=torch.int32, device=self.device)
            self._found_host = torch.zeros(self.max_batch, dtype=torch.int32).pin_memory()
        ptrs = (C.c_void_p * E)(*[mp[0].data_ptr() for mp in maps])
        ps = (C.c_longlong * E)(*[mp[1] for mp in maps])
        rs = (C.c_longlong * E)(*[mp[2] for mp in maps])
        params = (C.c_int * (6 * E))(*[v for mp in maps for v in mp[3]])
        outs = (C.c_void_p * E)(*[mp[4].data_ptr() for mp in maps])
        with torch.cuda.device(self.device):
            rc = _lib.load().peanut_goal_map_batch(E, ptrs, int(lm0.shape[0]), int(lm0.shape[1]), ps, rs, params, outs,
                                                   self._found_dev.data_ptr(), _lib.current_stream_ptr(self.device))
            _lib.check(rc, "peanut_goal_map_batch")
            self._found_host[:E].copy_(self._found_dev[:E], non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()
        return [int(v) for v in self._found_host[:E]]

    def _predict_batch(self, crops):
        """One prediction forward over the windows of the episodes that predict on this step -> [n,K,W,W]."""
        return self.active[0].prediction_model.get_prediction_batch(torch.cat(crops))

    # ---- host logic ----
    def drop(self, state):
        """Take an episode (the state or its index in ``active``) out of the batch."""
        if isinstance(state, int):
            del self.active[state]
        else:
            self.active.remove(state)

    def reset_active(self):
        self.active = list(self.states)

    def _check_batch(self, obs, infos):
        E = len(self.active)
        if E == 0:
            raise ValueError("no active episode")
        if len(infos) != E:
            raise ValueError(f"{len(infos)} infos for {E} active episodes")
        if obs.shape[0] != E:
            raise ValueError(f"obs holds {obs.shape[0]} frames for {E} active episodes")
        return E

    def init_with_obs(self, obs, infos):
        """``Agent_State.init_with_obs`` for every active episode: obs [E,C,h,w], E infos."""
        E = self._check_batch(obs, infos)
        for s in self.active:
            s.l_step = 0
            s.step = 0
        locs = self._map_step(obs, self._upload_poses([i['sensor_pose'] for i in infos]))
        for e, s in enumerate(self.active):
            s.locs = locs[e]
            r, c = s.locs[1], s.locs[0]
            loc_r, loc_c = [int(r * 100.0 / s.args.map_resolution), int(c * 100.0 / s.args.map_resolution)]
            s.local_map[2:4, loc_r - 1:loc_r + 2, loc_c - 1:loc_c + 2] = 1.
            rgoal = [0.1, 0.1]
            s.global_goals = [[int(rgoal[0] * s.local_w), int(rgoal[1] * s.local_h)]]
            s.global_goals = [[min(x, int(s.local_w - 1)), min(y, int(s.local_h - 1))] for x, y in s.global_goals]

    def update_goal_maps(self, states, infos):
        """``Agent_State.update_goal_map`` for the episodes of ``states`` that have ``args.goal_map`` on: one batched call (the
        episodes may differ in goal category, in the tv rule and in their strides), one read-back."""
        on = [(s, i) for s, i in zip(states, infos) if getattr(s.args, "goal_map", False)]
        if not on:
            return
        maps = []
        for s, i in on:
            mp = s._goal_map_args(i)
            if tuple(mp[0].shape) != tuple(on[0][0].local_map.shape):
                raise ValueError("update_goal_maps: the local maps of one batch must have one shape")
            maps.append(mp + (s.goal_map,))
        self.goal_map_batches += 1
        for (s, _), found in zip(on, self._goal_map_batch(maps)):
            s.found_goal = found

    def update_local_maps(self, obs, sensor_poses):
        """``Agent_State.update_local_map`` for every active episode: one pose upload, one projection, one read-back, the
        host decisions per episode, one marking launch."""
        act = list(self.active)
        locs = self._map_step(obs, self._upload_poses(sensor_poses))
        marks, cells = [], []
        for e, s in enumerate(act):
            loc_r, loc_c, traj_rad, centres = s._local_map_host(locs[e])
            marks.append(s._mark_args(loc_r, loc_c, traj_rad, centres) + (centres,))
            cells.append((loc_r, loc_c))
        self._mark_agent_batch(marks)
        for s, (loc_r, loc_c) in zip(act, cells):
            s.loc_r, s.loc_c = loc_r, loc_c

    def update_state(self, obs, infos):
        """``Agent_State.update_state`` for every active episode: obs [E,C,h,w], E infos.  Returns E flags: predicted."""
        E = self._check_batch(obs, infos)
        act = list(self.active)
        for s, i in zip(act, infos):
            s.goal_cat = i['goal_cat_id']
        self.update_local_maps(obs, [i['sensor_pose'] for i in infos])
        predicted = [False] * E
        batch = self._goal_batch([s for s in act if s._prediction_due()]) if self.batch_goals else []
        if batch:
            return self._update_state_goal_batch(act, batch, infos)
        if not self.batch_predictions:
            # the goal maps go through one call after the last episode's goal is final: only then are the step counters held back
            goal_maps = any(getattr(s.args, "goal_map", False) for s in act)
            for e, s in enumerate(act):
                s._step_full_map()
                if s._prediction_due():
                    select = getattr(s.args, "select_goal", True)
                    s.update_prediction(goal_follows=select)
                    if select:
                        s.update_global_goal()
                    predicted[e] = True
                if not goal_maps:
                    s.inc_step()
            if goal_maps:
                self.update_goal_maps(act, infos)
                for s in act:
                    s.inc_step()
            return predicted
        for s in act:
            s._step_full_map()
        due = [e for e, s in enumerate(act) if s._prediction_due()]
        if due:
            crops = [act[e]._prediction_input(getattr(act[e].args, "select_goal", True)) for e in due]
            preds = self._predict_batch(crops)
            for k, e in enumerate(due):
                act[e]._prediction_output(preds[k])
                if getattr(act[e].args, "select_goal", True):
                    act[e].update_global_goal()
                predicted[e] = True
        self.update_goal_maps(act, infos)
        for s in act:
            s.inc_step()
        return predicted

    def _update_state_goal_batch(self, act, batch, infos):
        """The rest of ``update_state`` on a step on which the episodes of ``batch`` (>= 2) select their goals in one solve: local
        periods, write-back of the batch's local maps, ONE begin, the prediction forwards (the batch's beside their E fields), the
        single way for the other due episodes, ONE ``select_batch``, the host bookkeeping per episode."""
        predicted = [False] * len(act)
        for s in act:
            s._step_full_map()
        due = [e for e, s in enumerate(act) if s._prediction_due()]
        in_batch = {id(s) for s in batch}
        for s in batch:
            s.full_map[:, s.lmb[0]:s.lmb[1], s.lmb[2]:s.lmb[3]] = s.local_map
        if getattr(batch[0].args, "goal_overlap", True):
            self._goal_begin_batch(batch)
        if not self.batch_predictions:
            for e in due:
                s = act[e]
                if id(s) in in_batch:
                    s._prediction_output(s.prediction_model.get_prediction_batch(s._prediction_crop())[0])
                else:
                    select = getattr(s.args, "select_goal", True)
                    s.update_prediction(goal_follows=select)
                    if select:
                        s.update_global_goal()
                predicted[e] = True
        else:
            crops = [act[e]._prediction_crop() if id(act[e]) in in_batch else
                     act[e]._prediction_input(getattr(act[e].args, "select_goal", True)) for e in due]
            preds = self._predict_batch(crops)
            for k, e in enumerate(due):
                act[e]._prediction_output(preds[k])
                if id(act[e]) not in in_batch and getattr(act[e].args, "select_goal", True):
                    act[e].update_global_goal()
                predicted[e] = True
        self.goal_batches += 1
        for s, res in zip(batch, self._goal_select_batch(batch)):
            s._goal_result(res)
        self.update_goal_maps(act, infos)
        for s in act:
            s.inc_step()
        return predicted

    def short_term_goals(self, infos, states=None):
        """``Agent_State.short_term_goal`` for the active episodes (or ``states``, a subset of them in their order; ``infos`` one per
        episode) that have ``args.plan_stg`` on -> one ``((stg_x, stg_y), stop)`` per episode, None for an episode with it off.
        With ``batch_stg`` the episodes that share a planner shape (``_stg_batch``) go through ONE ``get_stg_batch`` per group of
        ``STG_BATCH_MIN`` or more: the launches and synchronisations of the longest chain of solves among them instead of all chains in
        a row; every episode gets the bits of its own ``short_term_goal``, which is what a smaller group calls.  Sets ``stg`` and
        ``stg_stop`` of each state; raises where the single method raises."""
        act = list(self.active) if states is None else list(states)
        if len(infos) != len(act):
            raise ValueError(f"{len(infos)} infos for {len(act)} episodes")
        info_of = {id(s): i for s, i in zip(act, infos)}
        on = [s for s in act if getattr(s.args, "plan_stg", False)]
        if act and not on:
            raise RuntimeError("short_term_goals is behind args.plan_stg (default off): no episode has it on")
        for s in on:
            if s.goal_map is None:
                raise RuntimeError("short_term_goal needs update_goal_map (args.goal_map) to have run on this step")
        for group in (self._stg_batch(on) if self.batch_stg else [[s] for s in on]):
            if len(group) < self.STG_BATCH_MIN:
                for s in group:
                    s.short_term_goal(info_of[id(s)])
                continue
            from .planner import get_stg_batch
            res = get_stg_batch([s._stg_planner() for s in group], [s._stg_inputs(info_of[id(s)]) for s in group])
            self.stg_batches += 1
            for s, (stg, stop) in zip(group, res):
                s.stg, s.stg_stop = stg, stop
        return [(s.stg, s.stg_stop) if getattr(s.args, "plan_stg", False) else None for s in act]

    def plan_acts(self, infos, states=None):
        """``Agent_Helper.plan_act`` for the active episodes (or ``states``, a subset of them in their order; ``infos`` one per
        episode) on this step's planner inputs -> one ``{'action': a}`` per episode.  Every state needs its ``Agent_Helper``
        (``state.helper``) and ``update_goal_map`` to have run on this step.  The episodes that share a planner shape go through
        ``agent_helper.plan_act_batch``: their marks in ONE ``peanut_plan_mark_batch``, their short-term goals in ONE
        ``get_stg_batch``; every action, counter and map equals E single ``plan_act`` calls bit for bit.  An episode that is over
        (its ``timestep`` passed the limit) is simply not passed."""
        from .agent_helper import plan_act_batch
        act = list(self.active) if states is None else list(states)
        if len(infos) != len(act):
            raise ValueError(f"{len(infos)} infos for {len(act)} episodes")
        for s in act:
            if getattr(s, "helper", None) is None:
                raise RuntimeError("plan_acts needs an Agent_Helper per state (agent_helper.Agent_Helper(args, state))")
        inputs = {id(s): s.planner_inputs(i, host=False) for s, i in zip(act, infos)}
        out = {}
        for group in self._stg_batch(act):
            for s, a in zip(group, plan_act_batch([s.helper for s in group], [inputs[id(s)] for s in group])):
                out[id(s)] = a
            self.plan_batches += 1
        return [out[id(s)] for s in act]

    STG_BATCH_MIN = 2      # the smallest group that goes through get_stg_batch: the batch is faster from E = 2 on (5.5 -> 3.9 ms at 480^2, profiles/stg/stg_batch.jsonl)

    @staticmethod
    def _stg_batch(states):
        """The episodes split into the groups one ``get_stg_batch`` can take: equal local map size, full map size, ``col_rad`` and
        planner step size, in the order of their first members, at most ``planner.MAX_BATCH`` each."""
        from .planner import MAX_BATCH
        def key(s):
            return (s.local_w, s.local_h, s.full_w, s.full_h, int(s.args.col_rad), int(getattr(getattr(s, "_stg", None), "step_size", 5)))
        groups = {}
        for s in states:
            groups.setdefault(key(s), []).append(s)
        return [g[k:k + MAX_BATCH] for g in groups.values() for k in range(0, len(g), MAX_BATCH)]

    @staticmethod
    def _goal_batch(due_states):
        """The episodes of this step whose goals go through one batched solve: those with ``select_goal`` on that agree with the
        first such episode in what the batch call takes once (``dist_weight_temperature``, ``map_resolution``, ``goal_overlap``) and
        in the map size; fewer than two -> none (they go the single way)."""
        from .goal import MAX_BATCH
        def key(s):
            return (float(getattr(s.args, "dist_weight_temperature", 500)), int(s.args.map_resolution),
                    bool(getattr(s.args, "goal_overlap", True)), s.full_w, s.full_h, s.local_w, s.local_h, int(s.args.col_rad))
        sel = [s for s in due_states if getattr(s.args, "select_goal", True)]
        sel = [s for s in sel if key(s) == key(sel[0])][:MAX_BATCH]
        return sel if len(sel) >= 2 else []
