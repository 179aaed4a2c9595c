"""Habitat-free counterpart of the reference's agent facade ``PEANUT_Agent`` (nav/agent/peanut_agent.py:15-95):
same ``reset`` / ``act`` / ``get_info`` / ``get_sim_location`` / ``get_pose_change`` surface and call order,
driven by recorded observation tuples instead of a live ``habitat.Env``.

Per step (peanut_agent.py:38-68): pose change from ``gps`` / ``compass`` -> goal id through ``hm3d_to_coco``
(constants.py:23-31) -> segmentation + observation formatting (``Agent_Helper.preprocess_inputs``,
agent_helper.py:166-195; here the HIP detector / mask accumulation / ``peanut_preprocess_obs``) ->
``Agent_State.init_with_obs`` on the first frame -> ``Agent_State.update_state`` -> ``Agent_Helper.plan_act``
(agent_helper.py:130-159).  The last step is behind ``args.plan_act`` (a peanut_amd-only switch, default off; needs
``args.goal_map`` and ``args.plan_stg``): with it ``act`` returns the reference's ``'action'`` beside what it returns without it --
the planner inputs themselves (with ``args.goal_map`` on, the reference's whole planner-input dict under ``'planner_inputs'``;
with ``args.plan_stg`` on, also what ``_plan`` gets from ``_get_stg`` on them, under ``'stg'`` and ``'stop'``:
``Agent_State.short_term_goal``).  With ``plan_act`` on, ``'stg'`` and ``'stop'`` are those of the planner's own solve, which
sees this step's visited line and collision cells."""
from __future__ import annotations

from typing import Callable, Dict, Optional

import numpy as np
import torch

from .agent_helper import Agent_Helper, preprocess_obs
from .agent_state import Agent_State
from .pose import PoseTracker
from .segmentation import accumulate_instances

# nav/constants.py:21-31
hm3d_names = {0: "chair", 1: "bed", 2: "plant", 3: "toilet", 4: "tv_monitor", 5: "sofa"}
hm3d_to_coco = {0: 0, 1: 3, 2: 2, 3: 4, 4: 5, 5: 1}
# goal_cat_id (the COCO-side category the maps are indexed by) -> goal_name: the inverse of the two tables above, for drivers that
# start from the category (replay.run_episode / run_episodes); update_goal_map's tv rule reads the name
coco_goal_names = {coco: hm3d_names[hm3d] for hm3d, coco in hm3d_to_coco.items()}


class PEANUT_Agent:
    def __init__(self, args, task_config=None, detector: Optional[Callable] = None, prediction_model=None,
                 state_dict=None):
        """``detector``: callable(img_bgr uint8 [H,W,3] HIP tensor) -> (masks, classes, scores), e.g.
        ``peanut_amd.segmentation.HipDetector``; without one the observations must carry canned ``instances``
        (peanut_amd/episodes.py) or a ready ``obs`` tensor."""
        self.args = args
        self.agent_states = Agent_State(args, prediction_model=prediction_model, state_dict=state_dict)
        self.device = self.agent_states.device
        self.agent_helper = None
        if getattr(args, "plan_act", False):                               # peanut_agent.py:23-24
            if not (getattr(args, "goal_map", False) and getattr(args, "plan_stg", False)):
                raise ValueError("args.plan_act needs args.goal_map and args.plan_stg (the planner reads the goal map and the short-term goal)")
            self.agent_helper = Agent_Helper(args, self.agent_states)
        self.detector = detector
        self.pose = PoseTracker()
        self.first_obs = True
        self.total_episodes = 0
        self.timestep = 0
        self.goal_cat = -1

    # ---- peanut_agent.py:29-36 ----
    def reset(self):
        self.agent_states.reset()
        if self.agent_helper is not None:
            self.agent_helper.reset()
        self.pose.reset()
        self.first_obs = True
        self.step = 0
        self.timestep = 0
        self.total_episodes += 1

    @property
    def last_sim_location(self):
        return self.pose.last_sim_location

    # ---- peanut_agent.py:70-95 ----
    def get_info(self, obs):
        return self.pose.get_info(obs)

    def get_sim_location(self, obs):
        return self.pose.get_sim_location(obs)

    def get_pose_change(self, obs):
        return self.pose.get_pose_change(obs)

    # ---- Agent_Helper.preprocess_inputs (agent_helper.py:166-195) on the device ----
    def _preprocess(self, observations: Dict, goal_cat: int) -> torch.Tensor:
        if "obs" in observations:
            return observations["obs"].to(self.device)
        args = self.args
        rgb = torch.as_tensor(np.ascontiguousarray(observations["rgb"])).to(self.device)
        depth = torch.as_tensor(np.ascontiguousarray(observations["depth"], dtype=np.float32)).to(self.device)
        if "instances" in observations:
            masks, classes, scores = (torch.as_tensor(np.ascontiguousarray(a)).to(self.device) for a in observations["instances"])
        elif self.detector is not None:
            masks, classes, scores = self.detector(rgb.flip(-1))                       # RGB -> BGR (segmentation.py:44)
        else:
            raise ValueError("observation carries no instances and the agent has no detector")
        sem = accumulate_instances(masks, classes, scores, args.num_sem_categories - 1, args.sem_pred_prob_thr,
                                   args.goal_thr, goal_cat)
        return preprocess_obs(rgb, depth, sem, args)

    # ---- peanut_agent.py:38-68 ----
    def act(self, observations: Dict):
        self.timestep += 1
        if self.timestep > getattr(self.args, "timestep_limit", 499):     # always stop at episode end
            return {'action': 0}
        goal = int(np.asarray(observations['objectgoal']).reshape(-1)[0])
        info = self.get_info(observations)
        info['goal_name'] = hm3d_names[goal]
        goal = hm3d_to_coco[goal]
        self.goal_cat = goal                                               # Agent_Helper.set_goal_cat
        if self.agent_helper is not None:
            self.agent_helper.set_goal_cat(goal)
        obs = self._preprocess(observations, goal)
        if self.agent_helper is not None and getattr(self.args, "visualize", 0):
            self.agent_helper.rgb_vis = observations.get("rgb")            # agent_helper.py:222
        info['goal_cat_id'] = goal
        if self.first_obs:
            self.agent_states.init_with_obs(obs, info)
            self.first_obs = False
        predicted = self.agent_states.update_state(obs, info)
        st = self.agent_states
        out = {'predicted': bool(predicted), 'sensor_pose': info['sensor_pose'], 'goal_name': info['goal_name'],
               'pose_pred': st.planner_pose_inputs.copy(), 'global_goals': [list(g) for g in st.global_goals]}
        if getattr(self.args, "goal_map", False):                          # what Agent_Helper.plan_act takes (peanut_agent.py:66)
            out['planner_inputs'] = st.planner_inputs(info)
        if getattr(self.args, "plan_stg", False):                          # what _plan gets from _get_stg (agent_helper.py:323)
            if not getattr(self.args, "goal_map", False):
                raise ValueError("args.plan_stg needs args.goal_map (the short-term goal reads the goal map)")
            if self.agent_helper is None:
                out['stg'], out['stop'] = st.short_term_goal(info)
        if self.agent_helper is not None:                                  # peanut_agent.py:66-68
            out.update(self.agent_helper.plan_act(st.planner_inputs(info, host=False)))
            out['stg'], out['stop'] = st.stg, st.stg_stop
        return out
