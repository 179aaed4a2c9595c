"""Host logic of Agent_State_Group without a device: the three device calls of the group (pose upload, forward_batch with
its read-back, mark_agent_batch) and the states' device-side methods are stubbed; what is left is who is in the batch, which
episode does what on which step, and the argument checks."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from peanut_amd import agent_state as AS


class FakeMapping:
    MAX_BATCH = 16

    def __init__(self):
        self.reserved = 0
        self.batches = []

    def reserve(self, n):
        self.reserved = max(self.reserved, n)


def _args(**over):
    return AS.default_args(select_goal=False, num_local_steps=4, update_goal_freq=3, **over)


def _state(args, name, log, mapping=None):
    """An Agent_State without its constructor (which needs a device): the attributes the group and the shared host halves
    read, with the device-side methods replaced by log entries."""
    s = object.__new__(AS.Agent_State)
    s.args, s.name, s.device = args, name, torch.device("cpu")
    s.local_w = s.local_h = 240
    s.local_map = torch.zeros(14, 240, 240)
    s.local_pose = torch.tensor([6.0, 6.0, 0.0])
    s.origins = np.zeros(3)
    s.planner_pose_inputs = np.zeros(7)
    s.global_goals = [[24, 24]]
    s.dist_to_goal = float("inf")
    s.l_step = s.step = 0
    s.prediction_model = object()
    s.sem_map_module = mapping or FakeMapping()
    s._selem_mask = torch.zeros(1)
    s.update_full_map = lambda: log.append((name, "full_map", s.step))
    s.update_prediction = lambda goal_follows=False: log.append((name, "predict", s.step))
    s.update_global_goal = lambda: log.append((name, "goal", s.step))
    return s


class Group(AS.Agent_State_Group):
    """The group with its device calls replaced: poses stay on the host, the projection moves every episode 10 cm along x."""
    @staticmethod
    def _pinned(n):
        return torch.zeros((n, 3))

    def _map_step(self, obs, poses):
        self.sem_map_module.batches.append([s.name for s in self.active])
        locs = []
        for e, s in enumerate(self.active):
            s.poses = poses[e]
            s.local_pose = s.local_pose + torch.tensor([0.1, 0.0, 0.0])
            locs.append(s.local_pose.numpy())
        return np.stack(locs)

    def _mark_agent_batch(self, marks):
        self.marked = [(mk[3], list(mk[4])) for mk in marks]


def _infos(n):
    return [{"sensor_pose": [0.1, 0.0, 0.0], "goal_cat_id": e} for e in range(n)]


def test_group_steps_its_active_episodes_and_lets_them_leave():
    log, mapping = [], FakeMapping()
    args = _args()
    states = [_state(args, n, log, mapping) for n in "abc"]
    states[1].step, states[1].l_step = 2, 2                   # episode b is two steps ahead: its periods fall on other steps
    grp = Group(states)
    assert mapping.reserved == 3 and all(s.sem_map_module is mapping for s in states)
    obs = torch.zeros(3, 14, 120, 160)
    flags = [grp.update_state(obs, _infos(3)) for _ in range(2)]
    # step 0 predicts for a and c (step == 0), b predicts at its step 2 (2 % 3 == 2) and rolls its local period at l_step 3
    assert flags == [[True, True, True], [False, False, False]]
    assert [x for x in log if x[1] == "full_map"] == [("b", "full_map", 3)]
    assert [s.goal_cat for s in states] == [0, 1, 2]
    assert grp.marked[0] == ((118, 123, 122, 127), [(120, 124)])       # after two steps: row int(6.0 * 20), column int(6.2 * 20); one centre
    grp.drop(states[1])
    assert [s.name for s in grp.active] == ["a", "c"]
    with pytest.raises(ValueError):
        grp.update_state(obs, _infos(3))                       # three frames for two active episodes
    with pytest.raises(ValueError):
        grp.update_state(obs[:2], _infos(3))
    n_before = len(mapping.batches)
    flags = grp.update_state(obs[:2], _infos(2))
    assert mapping.batches[n_before:] == [["a", "c"]] and flags == [True, True]           # step 2 of a and c: 2 % 3 == 2
    assert (states[0].step, states[1].step, states[2].step) == (3, 4, 3)
    grp.update_state(obs[:2], _infos(2))                       # l_step 3 of a and c: their local period, one step after b's
    assert [x for x in log if x[1] == "full_map"] == [("b", "full_map", 3), ("a", "full_map", 3), ("c", "full_map", 3)]
    grp.drop(0)
    grp.drop(0)
    with pytest.raises(ValueError):
        grp.update_state(obs[:0], [])
    grp.reset_active()
    assert len(grp.active) == 3


def test_group_marks_the_goal_when_an_episode_is_near_it():
    log = []
    args = _args()
    states = [_state(args, n, log) for n in "ab"]
    states[1].global_goals = [[121, 121]]                      # b stands next to its goal: two footprints, and it predicts
    grp = Group(states)
    flags = grp.update_state(torch.zeros(2, 14, 120, 160), _infos(2))
    assert [len(c) for _, c in grp.marked] == [1, 2] and grp.marked[1][1][1] == (121, 121)
    assert flags == [True, True]
    flags = grp.update_state(torch.zeros(2, 14, 120, 160), _infos(2))
    assert flags == [False, True]                              # step 1: only the episode within goal_reached_dist predicts


def test_group_refuses_what_it_cannot_batch():
    log = []
    a, b = _state(_args(), "a", log), _state(_args(), "b", log)
    with pytest.raises(ValueError, match="vision_range"):
        Group([a, _state(_args(vision_range=64), "c", log)])
    with pytest.raises(ValueError, match="reserve"):
        Group([a, b], max_batch=1)
    with pytest.raises(ValueError):
        Group([a, b], max_batch=17)
    with pytest.raises(ValueError):
        Group([])
    with pytest.raises(ValueError):
        Group([a, a])
    other = _state(_args(), "d", log)
    other.device = torch.device("meta")
    with pytest.raises(ValueError):
        Group([a, other])
    grp = Group([a, b], max_batch=4)
    assert grp.sem_map_module.reserved == 4
    with pytest.raises(ValueError):
        grp.init_with_obs(torch.zeros(3, 14, 120, 160), _infos(2))


def test_the_split_single_episode_step_keeps_its_order():
    """Agent_State.update_local_map after the split: map step, ONE read-back, host decisions, mark, in that order."""
    log = []
    s = _state(_args(), "a", log)
    s._map_step = lambda obs: log.append("map_step")
    s._mark_agent = lambda r, c, rad, centres: log.append(("mark", r, c, rad, list(centres)))
    s.update_local_map(None)
    assert log == ["map_step", ("mark", 120, 120, 2, [(120, 120)])]
    assert (s.loc_r, s.loc_c) == (120, 120) and s.planner_pose_inputs[0] == 6.0
