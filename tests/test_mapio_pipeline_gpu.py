"""The map-dataset path end to end: ``MapSequenceRecorder`` as the on_step hook of lock-step and single episodes against the host
route (``encode_map`` of a map copied down, collect_maps.py:67-87), and ``evaluate`` against the host route of the loss
(``model_input``, the same forward, the float64 loss on ``target_from_sequence``)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LENGTHS = (6, 3, 6)
GOALS = (1, 4, 2)
SAVE = (2, 4, 5)


def _episodes():
    """Three episodes of 6, 3 and 6 frames: the frame recipe of the lock-step tests (a depth plane with noise, three instance
    masks, a pose that moves and turns), built here."""
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


class _HostRecorder:
    """collect_maps.py:67-87 with the parent's host route: ``encode_map`` of the map copied down as fp32."""

    def __init__(self, states, save_steps):
        self.states, self.save_steps = list(states), list(save_steps)
        self.seq = [None] * len(self.states)

    def on_step(self, i, act, predicted):
        from peanut_amd import mapio
        if i + 1 not in self.save_steps:
            return
        for s in (act if isinstance(act, list) else [act]):
            e = self.states.index(s)
            if self.seq[e] is None:
                self.seq[e] = np.zeros((len(self.save_steps),) + tuple(s.full_map.shape), np.uint8)
            self.seq[e][self.save_steps.index(i + 1)] = mapio.encode_map(s.full_map.cpu())


def _args():
    from peanut_amd.agent_state import default_args
    # a 480 x 480 full map; the local map goes back into the full map every second step, so that the snapshots differ
    return default_args(only_explore=1, map_size_cm=2400, num_local_steps=2)


def test_recorder_in_lockstep_and_single_episodes_equals_the_host_route(tmp_path):
    from peanut_amd import mapio
    from peanut_amd.agent_state import Agent_State
    from peanut_amd.replay import run_episode, run_episodes
    args = _args()
    eps = _episodes()
    states = [Agent_State(args, prediction_model=None) for _ in LENGTHS]
    rec = mapio.MapSequenceRecorder(states, save_steps=SAVE)
    host = _HostRecorder(states, SAVE)

    def both(i, act, predicted):
        rec.on_step(i, act, predicted)
        host.on_step(i, act, predicted)
    run_episodes(states, eps, GOALS, on_step=both)
    assert rec.launches == 3                                             # one launch per save step, whatever E
    kept = []
    for e, s in enumerate(states):
        seq = rec.sequence(s)
        assert seq.dtype == np.uint8 and seq.shape == (3, 14, 480, 480)
        assert np.array_equal(seq, host.seq[e]), e
        assert rec.sums(s) == (int(np.sum(seq[:, 4:], dtype=np.uint64)), int(np.sum(seq[:, 1], dtype=np.uint64)))
        assert rec.keep(s) == mapio.keep_sequence(seq)
        kept.append(rec.keep(s))
    assert host.seq[0][0].any() and not np.array_equal(host.seq[0][0], host.seq[0][2])        # (real, differing snapshots)
    assert host.seq[1][0].any() and not host.seq[1][1:].any()            # the 3-frame episode: zeros after its end
    assert any(kept)
    for e, s in enumerate(states):
        p = str(tmp_path / f"f{e:05d}.npz")
        assert rec.save(s, p) == kept[e]
        if kept[e]:
            assert np.array_equal(mapio.load_map_sequence(p), host.seq[e])
    p = str(tmp_path / "forced.npz")
    assert rec.save(states[1], p, force=True) and np.array_equal(mapio.load_map_sequence(p), host.seq[1])

    # one episode under run_episode (on_step gets the state itself)
    st = Agent_State(args, prediction_model=None)
    rec1 = mapio.MapSequenceRecorder([st], save_steps=SAVE)
    host1 = _HostRecorder([st], SAVE)

    def both1(i, s, predicted):
        rec1.on_step(i, s, predicted)
        host1.on_step(i, s, predicted)
    run_episode(st, eps[0], goal_cat=GOALS[0], on_step=both1)
    assert np.array_equal(rec1.sequence(st), host1.seq[0])
    assert np.array_equal(rec1.sequence(st), host.seq[0])                # lock-step episodes end with the bits they have alone
    assert rec1.keep(st) == mapio.keep_sequence(host1.seq[0])
    p = str(tmp_path / "single.npz")
    assert rec1.save(st, p, force=True) and np.array_equal(mapio.load_map_sequence(p), host1.seq[0])


def test_evaluate_equals_the_host_route(tmp_path):
    from types import SimpleNamespace

    from peanut_amd import mapio
    from peanut_amd.prediction import PEANUT_Prediction_Model
    from peanut_amd.weights import PredCfg, make_seeded_state_dict
    S, K, T = 47, 6, 3
    rng = np.random.RandomState(2)
    maps = (rng.uniform(0, 1, (T, 14, S, S)) ** 3 * 255).astype(np.uint8)
    maps[:, 1] *= (rng.uniform(0, 1, (T, S, S)) > 0.6).astype(np.uint8)
    files = [str(tmp_path / "f00002.npz"), str(tmp_path / "f00001.npz")]
    np.savez_compressed(files[0], maps=maps)
    np.savez_compressed(files[1], maps=maps[:, :, ::-1].copy())
    model = PEANUT_Prediction_Model(SimpleNamespace(sem_gpu_id=0), state_dict=make_seeded_state_dict(PredCfg(), 0))
    t_indices = (0, 1, 2)
    got = mapio.evaluate(model, str(tmp_path), t_indices=t_indices)
    assert got["n_maps"] == 6 and len(got["loss_per_channel"]) == K

    total, bound = np.zeros(K), 0.0
    for f in sorted(files):
        seq = mapio.load_map_sequence(f)
        dev = mapio.to_device(seq, model.model.device)
        # the host route: fp32 made on the host and uploaded, the same forward (one batch per file, as evaluate runs it)
        x = torch.cat([mapio.model_input(seq, t, device=model.model.device) for t in t_indices])
        assert torch.equal(mapio.model_input_batch(dev, t_indices), x)
        logits = model.get_prediction_batch(x, apply_sigmoid=False)
        assert torch.equal(model.get_prediction_batch(mapio.model_input_batch(dev, t_indices), apply_sigmoid=False), logits)
        for b, t in enumerate(t_indices):
            xs = logits[b].cpu().numpy().astype(np.float64)
            tgt = mapio.target_from_sequence(seq, t, range(4, 4 + K)).transpose(2, 0, 1)
            y = (tgt.astype(np.float32) / np.float32(255)).astype(np.float64)
            cell = (1 - y) * xs + np.maximum(-xs, 0) + np.log1p(np.exp(-np.abs(xs)))
            total += np.array([math.fsum(cell[k].reshape(-1).tolist()) for k in range(K)])
            bound += 64 * 2.0 ** -53 * float(np.sum(np.abs(xs) + 1))
    cells = 6 * S * S
    want = total / cells
    assert np.abs(np.array(got["loss_per_channel"]) - want).max() <= bound / cells
    assert abs(got["loss"] - want.mean()) <= bound / cells
    one = mapio.evaluate(model, [files[1]], t_indices=(1,), batch=1)
    assert one["n_maps"] == 1 and math.isfinite(one["loss"])
