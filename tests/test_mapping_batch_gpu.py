"""The batched stage 2 (peanut_map_forward_batch / peanut_map_mark_agent_batch / peanut_preprocess_obs_batch) against the
single-episode entry points: bit equality per episode, no tolerance of its own.  The single-episode path is what the
existing tests hold to the goldens made by the reference's own Semantic_Mapping (tests/test_mapping_gpu.py)."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _args(**over):
    a = dict(device=torch.device("cuda:0"), frame_height=120, frame_width=160, map_resolution=5, map_size_cm=4800,
             global_downscaling=2, vision_range=100, hfov=79.0, du_scale=1, cat_pred_threshold=5.0, exp_pred_threshold=1.0,
             map_pred_threshold=0.1, num_sem_categories=10, camera_height=0.88)
    a.update(over)
    return SimpleNamespace(**a)


def _module(args, reserve=0):
    from peanut_amd.mapping import Semantic_Mapping
    sm = Semantic_Mapping(args).to(torch.device("cuda:0")).eval()
    if reserve:
        sm.reserve(reserve)
    return sm


def _episode(seed, n=8, shift=0):
    """(obs [n,14,120,160], rel [n,3]) of oracle.mapping_scenes.make_sequence(seed, n), rotated by `shift` frames."""
    from oracle import mapping_scenes
    frames = mapping_scenes.make_sequence(seed, n)
    frames = frames[shift:] + frames[:shift]
    obs = torch.from_numpy(np.stack([mapping_scenes.frame_to_obs(fr) for fr in frames]))
    rel = torch.from_numpy(np.stack([fr["pose"] for fr in frames]))
    return obs.cuda(), rel.cuda()


def _far_episode(n=8):
    """The all-far frame of test_empty_and_far_frames, n times."""
    from oracle import mapping_scenes
    obs = torch.zeros(n, 14, 120, 160)
    obs[:, 3] = mapping_scenes.FAR_CM
    return obs.cuda(), torch.tensor([0.1, 0.0, 0.2]).repeat(n, 1).cuda()


def _start(M, centre, seed=None, theta=0.0):
    maps = torch.zeros(14, M, M) if seed is None else torch.rand(14, M, M, generator=torch.Generator().manual_seed(seed))
    return maps.cuda(), torch.tensor([centre, centre, theta]).cuda()


def _single_runs(args, episodes, starts):
    """Every episode stepped alone on a module of its own: per episode and frame (fp_map_pred, map_pred, pose)."""
    out = []
    for (obs, rel), (maps, pose) in zip(episodes, starts):
        sm = _module(args)
        maps, pose, rec = maps.clone(), pose.clone(), []
        for i in range(obs.shape[0]):
            fp, maps, _, _ = sm(obs[i:i + 1], rel[i], maps, pose, None)
            rec.append((fp[0].clone(), maps, pose.clone()))
        out.append(rec)
    return out


def _batched_run(sm, episodes, starts, want, between=None):
    """The same episodes as one batch, state carried from frame to frame; after every frame each episode must have the bits of
    its single run."""
    E, n = len(episodes), episodes[0][0].shape[0]
    maps = [m.clone() for m, _ in starts]
    poses = torch.stack([p for _, p in starts]).contiguous()
    for i in range(n):
        obs = torch.stack([ep[0][i] for ep in episodes])
        rel = torch.stack([ep[1][i] for ep in episodes])
        fp, maps, pp, cur = sm.forward_batch(obs, rel, maps, poses)
        assert pp.data_ptr() == poses.data_ptr() == cur.data_ptr()           # in place, like forward
        for e in range(E):
            assert torch.equal(fp[e], want[e][i][0]), f"episode {e} frame {i}: fp_map_pred"
            assert torch.equal(maps[e], want[e][i][1]), f"episode {e} frame {i}: map_pred"
            assert torch.equal(poses[e], want[e][i][2]), f"episode {e} frame {i}: pose"
        if between is not None:
            between(i)
    return maps, poses


@pytest.fixture(scope="module")
def eight():
    """Eight episodes of eight frames at the default configuration and their single-episode runs.  make_sequence's frame 3
    takes the low-stairs branch and frame 5 has a far band; episode 1 is offset by three frames, so stairs and non-stairs
    frames meet in one batch.  Episode 3 is the all-far frame on a random previous map; episodes 4 and 5 are identical."""
    args = _args()
    episodes = [_episode(30), _episode(31, shift=3), _episode(32), _far_episode(), _episode(34), _episode(34), _episode(36),
                _episode(37)]
    starts = [_start(480, 12.0) for _ in range(8)]
    starts[3] = _start(480, 12.0, seed=9, theta=30.0)
    return args, episodes, starts, _single_runs(args, episodes, starts)


@pytest.mark.parametrize("E", [1, 3, 8])
def test_forward_batch_equals_separate_modules(eight, E):
    args, episodes, starts, want = eight
    sm = _module(args, reserve=E)
    maps, _ = _batched_run(sm, episodes[:E], starts[:E], want)
    if E == 8:
        assert torch.equal(maps[4], maps[5])                                # identical inputs: equal to each other too
        assert torch.equal(maps[3], starts[3][0])                           # the all-far frames left their map as it was
        assert float(want[0][-1][1][4:].sum()) > 0                          # (and the others did project something)


@pytest.mark.parametrize("over,M,centre", [(dict(du_scale=2), 480, 12.0), (dict(vision_range=64, map_size_cm=2400), 240, 6.0)])
def test_forward_batch_at_other_flags(over, M, centre):
    args = _args(**over)
    episodes = [_episode(40), _episode(41, shift=3), _episode(42)]
    starts = [_start(M, centre) for _ in range(3)]
    want = _single_runs(args, episodes, starts)
    sm = _module(args, reserve=3)
    _batched_run(sm, episodes, starts, want)
    assert sm.debug_launches() == (9 if args.du_scale > 1 else 8)


def test_forward_batch_repeats_permutes_and_coexists_with_forward(eight):
    """The same E = 3 batch twice gives the same bits; permuted episodes give permuted outputs and nothing else; a single
    `forward` on the same handle between two batched calls disturbs neither side."""
    args, episodes, starts, want = eight
    sm = _module(args, reserve=3)
    _batched_run(sm, episodes[:3], starts[:3], want)
    _batched_run(sm, episodes[:3], starts[:3], want)                         # again, on the handle's used slots
    perm = [2, 0, 1]
    _batched_run(sm, [episodes[p] for p in perm], [starts[p] for p in perm], [want[p] for p in perm])
    # a single-episode sequence (episode 6) interleaved, one frame after every batched frame, on the SAME handle
    obs6, rel6 = episodes[6]
    state = {"maps": starts[6][0].clone(), "pose": starts[6][1].clone()}

    def single_step(i):
        fp, state["maps"], _, _ = sm(obs6[i:i + 1], rel6[i], state["maps"], state["pose"], None)
        assert torch.equal(fp[0], want[6][i][0]) and torch.equal(state["maps"], want[6][i][1])
        assert torch.equal(state["pose"], want[6][i][2])
    _batched_run(sm, episodes[:3], starts[:3], want, between=single_step)


def test_forward_batch_golden_sequences(golden_dir):
    """The default-configuration sequences of mapping_golden.npz as one batch (shorter ones leave as they end) meet the gates
    of test_golden_sequences as that test states them: fp_map_pred bits exact, poses 1e-5, final map VAL_TOL."""
    from test_mapping_gpu import VAL_TOL
    assert VAL_TOL == 3.5e-5
    z = np.load(os.path.join(golden_dir, "mapping_golden.npz"))
    names = [n for n in sorted({k.split("/")[0] for k in z.files})
             if z[f"{n}/depth"].shape[1:] == (120, 160) and z[f"{n}/sem"].shape[1] == 10]
    assert len(names) >= 2
    sm = _module(_args(), reserve=len(names))
    maps = {n: torch.zeros(14, 480, 480, device="cuda") for n in names}
    pose = {n: torch.tensor([12.0, 12.0, 0.0], device="cuda") for n in names}
    for i in range(max(z[f"{n}/depth"].shape[0] for n in names)):
        act = [n for n in names if i < z[f"{n}/depth"].shape[0]]
        obs = np.zeros((len(act), 14, 120, 160), np.float32)
        for e, n in enumerate(act):
            obs[e, 3] = z[f"{n}/depth"][i]
            obs[e, 4:] = z[f"{n}/sem"][i].astype(np.float32)
        rel = torch.from_numpy(np.stack([z[f"{n}/pose_obs"][i] for n in act])).cuda()
        poses = torch.stack([pose[n] for n in act]).contiguous()
        fp, out, _, _ = sm.forward_batch(torch.from_numpy(obs).cuda(), rel, [maps[n] for n in act], poses)
        for e, n in enumerate(act):
            maps[n], pose[n] = out[e], poses[e].clone()
            assert np.array_equal(np.packbits(fp[e].cpu().numpy().astype(bool)), z[f"{n}/fp_map_bits"][i]), f"{n} frame {i}"
            np.testing.assert_allclose(pose[n].cpu().numpy(), z[f"{n}/poses"][i], rtol=0, atol=1e-5)
    for n in names:
        final = maps[n].cpu().numpy().reshape(-1)
        ref = np.zeros_like(final)
        ref[z[f"{n}/final_idx"]] = z[f"{n}/final_val"]
        err = np.abs(final - ref).max()
        print(f"{n}: final map max-abs vs the reference golden {err:.3e}")
        assert err <= VAL_TOL, f"{n}: final map max-abs {err:.3e}"


def test_forward_batch_launches_and_refusals(eight):
    """One batched step at E = 8 enqueues as many kernels as one single step; E above the reserve, aliasing and shared outputs
    are refused before anything is enqueued."""
    from peanut_amd import _lib
    args, episodes, starts, want = eight
    sm = _module(args, reserve=8)
    obs = torch.stack([ep[0][0] for ep in episodes])
    rel = torch.stack([ep[1][0] for ep in episodes])
    maps = [m.clone() for m, _ in starts]
    poses = torch.stack([p for _, p in starts]).contiguous()
    sm(obs[:1], rel[0], maps[0], poses[0].clone(), None)
    single = sm.debug_launches()
    fp, out, _, _ = sm.forward_batch(obs, rel, maps, poses)
    assert sm.debug_launches() == single == 8
    # refusals: the outputs handed in stay as they were
    small = _module(args, reserve=2)
    with pytest.raises(ValueError):
        small.forward_batch(obs[:3], rel[:3], maps[:3], poses[:3].contiguous())          # E above the reserve
    with pytest.raises(ValueError):
        sm.forward_batch(obs[:3], rel[:3], maps[:2], poses[:3].contiguous())             # two maps for three episodes
    with pytest.raises(ValueError):
        sm.forward_batch(obs, rel[:, :2], maps, poses)
    lib = _lib.load()
    mark = [o.clone() for o in out[:3]]
    fp3 = torch.full((3, 100, 100), 7.0, device="cuda")
    p3 = poses[:3].clone()

    def call(E, last, pred):
        a = (C.c_void_p * len(last))(*[t.data_ptr() for t in last])
        b = (C.c_void_p * len(pred))(*[t.data_ptr() for t in pred])
        return lib.peanut_map_forward_batch(sm._h, E, obs.data_ptr(), rel.data_ptr(), a, p3.data_ptr(), fp3.data_ptr(), b,
                                            _lib.current_stream_ptr(obs.device))
    assert call(3, maps[:3], [out[0], out[1], out[1]]) == -2                            # two episodes share one output
    assert call(3, [maps[0], maps[1], out[2]], out[:3]) == -2                           # map_pred[2] is maps_last[2]
    assert call(9, maps[:3], out[:3]) == -2 and call(0, maps[:3], out[:3]) == -2
    assert lib.peanut_map_forward_batch(sm._h, 3, obs.data_ptr(), rel.data_ptr(), None, p3.data_ptr(), fp3.data_ptr(), None, None) == -2
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(mark, out[:3])) and bool((fp3 == 7.0).all()) and torch.equal(p3, poses[:3])
    assert call(3, maps[:3], out[:3]) == 0                                               # and the handle still works


def test_mark_agent_batch_equals_the_single_calls():
    """The cases of test_map_bookkeeping_in_one_launch_equals_the_tensor_operations (a square clamped at the border, two
    centres, zero centres among them), all in one launch, against one peanut_map_mark_agent call each; an out-of-range
    footprint in one episode refuses the whole call and leaves every map as it was."""
    from oracle.agent_ref import agent_args
    from peanut_amd import _lib
    from peanut_amd.agent_state import Agent_State, Agent_State_Group
    args = agent_args()
    st = Agent_State(args, prediction_model=None)
    m, off = st.local_w, int(args.col_rad + 1)
    g = torch.Generator().manual_seed(3)
    base = torch.rand((st.nc, m, m), generator=g).cuda()
    cases = [((240, 240), None), ((100, 377), (300, 20)), ((off, off), None), ((m - 1 - off, m - 1 - off), (off, m - 1 - off)),
             ((1, 2), None), ((0, m - off - 1), None), ((3, 3), (2, 1)), ((m - 1 - off, 0), None)]
    want, marks = [], []
    for loc, goal in cases:
        centres = [loc] + ([goal] if goal else [])
        st.local_map = base.clone()
        st._mark_agent(loc[0], loc[1], 2, centres)
        want.append(st.local_map)
        st.local_map = base.clone()
        marks.append(st._mark_args(loc[0], loc[1], 2, centres) + (centres,))
    st.local_map = base.clone()
    marks.append(st._mark_args(50, 60, 2, []) + ([],))                       # zero centres: only the square
    lm = base.clone()
    lm[2].fill_(0.)
    lm[2:4, 48:53, 58:63] = 1.
    want.append(lm)
    grp = Agent_State_Group([st], max_batch=1)
    grp.active = [st]
    grp._mark_agent_batch(marks)
    for k, mk in enumerate(marks):
        assert torch.equal(mk[0], want[k]), k
    # refusal: episode 1's footprint row reaches m
    lib = _lib.load()
    maps = [base.clone() for _ in range(3)]
    ptrs = (C.c_void_p * 3)(*[t.data_ptr() for t in maps])
    squares = (C.c_int * 12)(*([10, 15, 10, 15] * 3))
    n_c = (C.c_int * 3)(1, 1, 1)
    centres = (C.c_int * 12)(12, 12, 0, 0, m - 2, 100, 0, 0, 12, 12, 0, 0)
    rc = lib.peanut_map_mark_agent_batch(3, ptrs, st.nc, m, squares, st._selem_mask.data_ptr(), off, n_c, centres,
                                         _lib.current_stream_ptr(st.device))
    torch.cuda.synchronize()
    assert rc == -2 and all(torch.equal(t, base) for t in maps)
    same = (C.c_void_p * 3)(maps[0].data_ptr(), maps[1].data_ptr(), maps[0].data_ptr())
    ok_c = (C.c_int * 12)(12, 12, 0, 0, 12, 12, 0, 0, 12, 12, 0, 0)
    assert lib.peanut_map_mark_agent_batch(3, same, st.nc, m, squares, st._selem_mask.data_ptr(), off, n_c, ok_c,
                                           _lib.current_stream_ptr(st.device)) == -2      # two episodes, one map


def test_preprocess_obs_batch_equals_four_single_calls():
    """The input recipe of test_preprocess_obs_matches_reference_loop with four seeds: the batch equals four preprocess_obs
    calls bit for bit, and episode 0 equals the NumPy restatement of the reference as in that test."""
    from oracle.agent_ref import preprocess_obs_ref
    from peanut_amd.agent_helper import preprocess_obs, preprocess_obs_batch
    H, W, ncat = 480, 640, 10
    args = SimpleNamespace(env_frame_width=W, frame_width=160, min_depth=0.5, max_depth=5.0)
    rgbs, depths, sems = [], [], []
    for seed in range(4):
        rng = np.random.RandomState(seed)
        depth = rng.uniform(0.0, 1.1, size=(H, W, 1)).astype(np.float32)
        depth[rng.uniform(size=(H, W, 1)) < 0.1] = 0.0
        depth[:, 100:140] = 0.0
        depth[:470, 300:320] = 0.0
        depth[:, 500:520][depth[:, 500:520] > 0.5] = 0.995
        rgbs.append(rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8))
        depths.append(depth)
        sems.append((rng.uniform(size=(H, W, ncat)) > 0.9).astype(np.float32))
    rgb, depth, sem = (torch.from_numpy(np.stack(v)).cuda() for v in (rgbs, depths, sems))
    got = preprocess_obs_batch(rgb, depth, sem, args)
    assert got.shape == (4, 14, 120, 160)
    for e in range(4):
        assert torch.equal(got[e:e + 1], preprocess_obs(rgb[e], depth[e], sem[e], args)), e
    ref = preprocess_obs_ref(rgbs[0].astype(np.float32), depths[0].copy(), sems[0], args).astype(np.float32)
    assert np.array_equal(got[0].cpu().numpy(), ref)
    assert torch.equal(preprocess_obs_batch(rgb, depth[..., 0], sem, args), got)         # depth [E,H,W] as well
