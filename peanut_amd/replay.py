"""Habitat-free replay of the reference's episode/step loop (nav/collect.py:44-84 +
PEANUT_Agent.act, nav/agent/peanut_agent.py:38-68) over recorded -- or synthetic -- frame tuples:
per step  seg mask accumulation -> observation formatting -> map projection -> (every
update_goal_freq steps) map prediction, with episodes sharded over ranks exactly like the
reference's ``--start_ep/--end_ep`` flags.  Planning/acting needs the simulator and is not here."""
from __future__ import annotations

from typing import Callable, Dict, Iterable, List, Optional


from . import dist as pdist
from .agent_helper import preprocess_obs
from .agent_state import Agent_State
from .peanut_agent import coco_goal_names
from .segmentation import accumulate_instances


def run_episode(state: Agent_State, frames: Iterable[Dict], goal_cat: int,
                on_step: Optional[Callable[[int, Agent_State, bool], None]] = None, detector=None) -> int:
    """frames: dicts with either a ready ``obs`` [1,C,h,w] HIP tensor or the raw tuple
    (``rgb`` u8 [H,W,3], ``depth`` [H,W,1], and instance ``masks``/``classes``/``scores`` unless a ``detector``
    -- e.g. ``peanut_amd.segmentation.HipDetector`` -- is given, which is then run on the BGR-flipped frame as
    ``SemanticPredMaskRCNN.get_prediction`` does, segmentation.py:44-45), plus ``sensor_pose`` = (dx, dy, do)
    (peanut_agent.py:70-95).  Returns the number of predictions."""
    args = state.args
    state.reset()
    n_pred = 0
    for i, fr in enumerate(frames):
        if "obs" in fr:
            obs = fr["obs"]
        else:
            if "masks" not in fr and detector is None:
                raise ValueError("frame carries no instance masks and no detector was given")
            if "masks" not in fr and hasattr(detector, "semantic"):     # detector + accumulation in one library call
                sem = detector.semantic(fr["rgb"].flip(-1), args.num_sem_categories - 1, args.sem_pred_prob_thr, args.goal_thr,
                                        goal_cat)                       # RGB -> BGR
            else:
                if "masks" not in fr:
                    fr = dict(fr)
                    fr["masks"], fr["classes"], fr["scores"] = detector(fr["rgb"].flip(-1))
                sem = accumulate_instances(fr["masks"], fr["classes"], fr["scores"], args.num_sem_categories - 1,
                                           args.sem_pred_prob_thr, args.goal_thr, goal_cat)
            obs = preprocess_obs(fr["rgb"], fr["depth"], sem, args)
        infos = {"sensor_pose": fr["sensor_pose"], "goal_cat_id": goal_cat, "goal_name": coco_goal_names.get(int(goal_cat), "")}
        if i == 0:
            state.init_with_obs(obs, infos)
        predicted = state.update_state(obs, infos)
        n_pred += int(predicted)
        if on_step is not None:
            on_step(i, state, predicted)
    return n_pred


def run_episodes(states, episodes, goal_cats, detector=None,
                 on_step: Optional[Callable[[int, List[Agent_State], List[bool]], None]] = None,
                 batch_predictions: bool = False, batch_goals: bool = True, batch_stg: bool = True,
                 on_group: Optional[Callable] = None) -> List[int]:
    """``run_episode`` for E episodes in lock-step on one device (``Agent_State_Group``): ``states`` E ``Agent_State``
    objects with equal mapping arguments, ``episodes`` E frame sequences in the formats of ``run_episode``, ``goal_cats`` E
    goal categories.  Per step the frames of the episodes still running are formatted, projected and marked as one batch;
    with a ``detector`` that has ``semantic``, they go through ONE ``detector.semantic(rgb[E].flip(-1), ..., goal_cats)``
    call.  Episodes may differ in length: a finished one drops out and the others go on.  ``on_step(i, active_states,
    predicted)`` is called after every step.  ``batch_goals``: the episodes that select a goal on the same step do so in one batched
    solve (``Agent_State_Group``; the same bits as one by one); ``batch_stg``: likewise the short-term goals, for an ``on_step`` that
    asks the group for them (``group.short_term_goals(infos)``; ``on_group(group)`` hands the group over once, before the first step).
    Returns the number of predictions per episode."""
    import torch
    from .agent_helper import preprocess_obs_batch
    from .agent_state import Agent_State_Group
    states, goal_cats = list(states), [int(g) for g in goal_cats]
    iters = [iter(ep) for ep in episodes]
    if not (len(states) == len(iters) == len(goal_cats)):
        raise ValueError(f"{len(states)} states, {len(iters)} episodes and {len(goal_cats)} goal categories")
    group = Agent_State_Group(states, batch_predictions=batch_predictions, batch_goals=batch_goals, batch_stg=batch_stg)
    if on_group is not None:
        on_group(group)
    args = states[0].args
    for s in states:
        s.reset()
    n_pred = [0] * len(states)
    index = {id(s): e for e, s in enumerate(states)}
    i = 0
    while True:
        frames = []
        for s in list(group.active):
            fr = next(iters[index[id(s)]], None)
            if fr is None:
                group.drop(s)                      # this episode is over; the others go on
            else:
                frames.append(fr)
        if not group.active:
            break
        act = list(group.active)
        goals = [goal_cats[index[id(s)]] for s in act]
        if all("obs" in fr for fr in frames):
            obs = torch.cat([fr["obs"] for fr in frames])
        else:
            if any("obs" in fr for fr in frames):
                raise ValueError("the frames of one step mix ready observations and raw tuples")
            raw = [fr for fr in frames if "masks" not in fr]
            if raw and detector is None:
                raise ValueError("frame carries no instance masks and no detector was given")
            rgb = torch.stack([fr["rgb"] for fr in frames])
            depth = torch.stack([fr["depth"] for fr in frames])
            if len(raw) == len(frames) and hasattr(detector, "semantic"):      # detector + accumulation: one library call
                sem = detector.semantic(rgb.flip(-1), args.num_sem_categories - 1, args.sem_pred_prob_thr, args.goal_thr,
                                        goals)                                  # RGB -> BGR
            else:
                sems = []
                for fr, goal in zip(frames, goals):
                    if "masks" not in fr:
                        fr = dict(fr)
                        fr["masks"], fr["classes"], fr["scores"] = detector(fr["rgb"].flip(-1))
                    sems.append(accumulate_instances(fr["masks"], fr["classes"], fr["scores"], args.num_sem_categories - 1,
                                                     args.sem_pred_prob_thr, args.goal_thr, goal))
                sem = torch.stack(sems)
            obs = preprocess_obs_batch(rgb, depth, sem, args)
        infos = [{"sensor_pose": fr["sensor_pose"], "goal_cat_id": goal, "goal_name": coco_goal_names.get(goal, "")}
                 for fr, goal in zip(frames, goals)]
        if i == 0:
            group.init_with_obs(obs, infos)
        predicted = group.update_state(obs, infos)
        for s, p in zip(act, predicted):
            n_pred[index[id(s)]] += int(p)
        if on_step is not None:
            on_step(i, act, predicted)
        i += 1
    return n_pred


def run_recorded_episode(agent, episode, on_step: Optional[Callable[[int, Dict], None]] = None) -> int:
    """One pass of the reference's inner loop (nav/collect.py:44-59: ``hab_env.reset(); nav_agent.reset();
    while not episode_over: action = nav_agent.act(observations)``) over a recorded episode
    (peanut_amd/episodes.py: the (rgb, depth, gps, compass, objectgoal) tuples Habitat produced).  ``agent`` is a
    ``peanut_amd.peanut_agent.PEANUT_Agent``; ``episode`` a path or a loaded dict.  Returns the number of
    predictions."""
    from . import episodes as E
    ep = E.load_episode(episode) if isinstance(episode, str) else episode
    agent.reset()
    n_pred = 0
    for i, observations in enumerate(E.iter_observations(ep)):
        out = agent.act(observations)
        n_pred += int(out.get('predicted', False))
        if on_step is not None:
            on_step(i, out)
    return n_pred


def run_recorded_shard(agent, episode_paths: List[str], start_ep: int = 0, end_ep: int = -1,
                       on_episode: Optional[Callable[[int, int], None]] = None) -> Dict[int, int]:
    """The outer loop of nav/collect.py:40-84 with its ``--start_ep/--end_ep`` window (:37-39,50): every episode
    before ``end_ep`` is iterated (the reference resets the env for skipped ones too), only those in
    [start_ep, end_ep) are run.  Returns {episode index: predictions}."""
    num_episodes = len(episode_paths)
    end = end_ep if end_ep > 0 else num_episodes
    done = {}
    ep_i = 0
    while ep_i < min(num_episodes, end):
        if start_ep <= ep_i < end:
            done[ep_i] = run_recorded_episode(agent, episode_paths[ep_i])
            if on_episode is not None:
                on_episode(ep_i, done[ep_i])
        ep_i += 1
    return done


def episode_shard(n_episodes: int) -> List[int]:
    """Episode ids owned by this rank (contiguous ``[start_ep, end_ep)`` like nav/collect.py:50)."""
    rank, _, world = pdist.env_rank_world()
    s, e = pdist.shard_range(n_episodes, rank, world)
    return list(range(s, e))
