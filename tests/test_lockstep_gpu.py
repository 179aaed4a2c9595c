"""Lock-step episodes (peanut_amd.replay.run_episodes over Agent_State_Group) against the same episodes run one after the
other with run_episode: with the default batch-1 predictions every episode must end with the bits it has alone."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LENGTHS = (12, 9, 12)
GOALS = (1, 4, 2)


def _episodes():
    """Three episodes of 12, 9 and 12 frames (the frame recipe of test_replay_loop_runs_full_pipeline) with their own
    masks, poses and goal categories."""
    g = torch.Generator().manual_seed(0)
    eps = []
    for e, n in enumerate(LENGTHS):
        frames = []
        for i in range(n):
            depth = torch.full((480, 640, 1), 0.3 + 0.05 * e) + torch.rand((480, 640, 1), generator=g) * 0.01
            masks = torch.zeros((3, 480, 640), dtype=torch.bool)
            masks[0, 280:400, 100 + 40 * e:220 + 40 * e] = True
            masks[1, 150:260, 300:420] = True
            masks[2, 10:60, 500:600] = True
            frames.append(dict(rgb=torch.randint(0, 256, (480, 640, 3), generator=g, dtype=torch.uint8).cuda(),
                               depth=depth.cuda(), masks=masks.cuda(), classes=torch.tensor([1, 4, 2 + e]).cuda(),
                               scores=torch.tensor([0.99, 0.97, 0.5 + 0.25 * e]).cuda(),
                               sensor_pose=[0.1 + 0.02 * e, 0.01 * e, (0.05 if i % 3 else 0.0) * (1 - e)]))
        eps.append(frames)
    return eps


@pytest.fixture(scope="module")
def setup():
    from oracle.agent_ref import agent_args
    from peanut_amd.agent_state import Agent_State
    from peanut_amd.prediction import PEANUT_Prediction_Model
    from peanut_amd.replay import run_episode
    from peanut_amd.weights import PredCfg, make_seeded_state_dict
    # (beyond the configuration of test_replay_loop_runs_full_pipeline: goal selection on, and num_local_steps = 5 so that the local
    # period -- update_full_map -- falls inside these short episodes)
    args = agent_args(only_explore=0, prediction_window=240, map_size_cm=2400, select_goal=True, num_local_steps=5)
    model = PEANUT_Prediction_Model(args, state_dict=make_seeded_state_dict(PredCfg(), 0))
    eps = _episodes()
    alone, counts, steps = [], [], []
    for frames, goal in zip(eps, GOALS):
        st = Agent_State(args, prediction_model=model)
        mine = []
        counts.append(run_episode(st, frames, goal_cat=goal, on_step=lambda i, s, p, mine=mine: mine.append(bool(p))))
        alone.append(st)
        steps.append(mine)
    return args, model, eps, alone, counts, steps


def _new_states(args, model, n=3):
    from peanut_amd.agent_state import Agent_State
    return [Agent_State(args, prediction_model=model) for _ in range(n)]


def test_run_episodes_equals_sequential_run_episode(setup):
    from peanut_amd.replay import run_episodes
    args, model, eps, alone, counts, steps = setup
    states = _new_states(args, model)
    seen = [[] for _ in states]
    sizes = []

    def on_step(i, act, predicted):
        sizes.append(len(act))
        for s, p in zip(act, predicted):
            seen[states.index(s)].append(bool(p))
    got = run_episodes(states, eps, GOALS, on_step=on_step)
    assert got == counts and all(c >= 1 for c in counts)
    assert seen == steps
    assert sizes == [3] * 9 + [2] * 3                       # the 9-frame episode left, the others went on
    for e, (a, b) in enumerate(zip(states, alone)):
        assert torch.equal(a.full_map, b.full_map), e
        assert torch.equal(a.local_map, b.local_map), e
        assert torch.equal(a.local_pose, b.local_pose) and torch.equal(a.full_pose, b.full_pose), e
        assert list(a.lmb) == list(b.lmb) and a.global_goals == b.global_goals, e
        assert torch.equal(a.target_pred, b.target_pred), e
        assert (a.step, a.l_step, a.loc_r, a.loc_c) == (b.step, b.l_step, b.loc_r, b.loc_c), e
        assert float(a.local_map[4:].sum()) > 0
    assert not torch.equal(states[0].local_map, states[2].local_map)      # (the episodes are different episodes)
    with pytest.raises(ValueError):
        run_episodes(states, eps[:2], GOALS)


def test_batched_predictions_stay_within_the_batched_forward_tolerance(setup):
    """batch_predictions=True: the same steps predict; target_pred is within the 2e-5 that
    test_batch_independence_and_determinism grants a batched forward on LOGITS (the sigmoid's slope is at most 1/4, so
    the bound only shrinks on probabilities).  Goal cells are printed, not asserted."""
    from peanut_amd.replay import run_episodes
    args, model, eps, alone, counts, steps = setup
    states = _new_states(args, model)
    seen = [[] for _ in states]

    def on_step(i, act, predicted):
        for s, p in zip(act, predicted):
            seen[states.index(s)].append(bool(p))
    got = run_episodes(states, eps, GOALS, on_step=on_step, batch_predictions=True)
    assert got == counts and seen == steps
    for e, (a, b) in enumerate(zip(states, alone)):
        err = (a.target_pred - b.target_pred).abs().max().item()
        print(f"episode {e}: target_pred max-abs vs batch-1 predictions {err:.3e}; goal {a.global_goals} vs {b.global_goals}")
        assert err <= 2e-5, (e, err)
        assert torch.equal(a.local_map, b.local_map), e       # the maps do not depend on the prediction


def test_run_episodes_with_the_detector_adds_only_the_flip():
    """Detector in the loop (the small seeded detector and thresholds of test_replay_loop_with_the_hip_detector), E = 2,
    4 frames: raw frames through run_episodes(detector=det) equal frames whose ready `obs` were built here from one
    det.semantic call at B = 2 per step and preprocess_obs_batch."""
    from oracle.agent_ref import agent_args
    from peanut_amd.agent_helper import preprocess_obs_batch
    from peanut_amd.agent_state import Agent_State
    from peanut_amd.prediction import PEANUT_Prediction_Model
    from peanut_amd.rcnn_weights import RcnnCfg, make_seeded_rcnn_state_dict
    from peanut_amd.replay import run_episodes
    from peanut_amd.segmentation import HipDetector
    from peanut_amd.weights import PredCfg, make_seeded_state_dict
    rcfg = RcnnCfg(depth=50, min_size=128, max_size=256, rpn_pre_nms_topk=60, rpn_post_nms_topk=40,
                   detections_per_image=10, score_thresh_test=0.15)
    det = HipDetector(rcfg, make_seeded_rcnn_state_dict(rcfg, 7))
    args = agent_args(only_explore=0, prediction_window=240, map_size_cm=2400, sem_pred_prob_thr=0.205, goal_thr=0.212)
    model = PEANUT_Prediction_Model(args, state_dict=make_seeded_state_dict(PredCfg(), 0))
    goals = [5, 3]
    g = torch.Generator().manual_seed(3)
    raw = [[], []]
    for i in range(4):
        for e in range(2):
            depth = torch.full((480, 640, 1), 0.3) + torch.rand((480, 640, 1), generator=g) * 0.01
            raw[e].append(dict(rgb=torch.randint(0, 256, (480, 640, 3), generator=g, dtype=torch.uint8).cuda(), depth=depth.cuda(),
                               sensor_pose=[0.1, 0.02 * e, 0.0]))
    ready = [[], []]
    calls = []
    for i in range(4):
        rgb = torch.stack([raw[e][i]["rgb"] for e in range(2)])
        sem = det.semantic(rgb.flip(-1), args.num_sem_categories - 1, args.sem_pred_prob_thr, args.goal_thr, goals)
        assert sem.shape == (2, 480, 640, args.num_sem_categories)
        obs = preprocess_obs_batch(rgb, torch.stack([raw[e][i]["depth"] for e in range(2)]), sem, args)
        for e in range(2):
            ready[e].append(dict(obs=obs[e:e + 1].clone(), sensor_pose=raw[e][i]["sensor_pose"]))
    inner = det.net.semantic

    def counted(img, *a, **k):
        calls.append(tuple(img.shape))
        return inner(img, *a, **k)
    det.net.semantic = counted
    a = [Agent_State(args, prediction_model=model) for _ in range(2)]
    b = [Agent_State(args, prediction_model=model) for _ in range(2)]
    try:
        assert run_episodes(a, raw, goals, detector=det) == run_episodes(b, ready, goals) == [1, 1]
    finally:
        det.net.semantic = inner
    assert calls == [(2, 480, 640, 3)] * 4                    # one detector call per step, both frames in it
    for e in range(2):
        assert float(a[e].local_map[4:].sum()) > 0            # detections reached the maps
        assert torch.equal(a[e].local_map, b[e].local_map) and torch.equal(a[e].full_map, b[e].full_map)
        assert torch.equal(a[e].target_pred, b[e].target_pred)
    with pytest.raises(ValueError):
        run_episodes(a, raw, goals)                           # no masks and no detector
