"""The edge scenes of oracle/mapping_scenes.py are what they claim to be -- checked with the CPU oracle alone, so the GPU
tests that run them (tests/test_mapping_edges_gpu.py) need no trust: every stairs pair sits on both sides of mapping.py:94
by exactly the designed counts, the dense frames have cells with hundreds of points whose summation order matters, the
limit frames touch and cross every face of the voxel grid, the heading wraps, and the border starts cut the window.
Also holds mapping_golden_edges.npz to the scenes it was made from and the restatement to the reference's stored bits."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import mapping_ref, mapping_scenes

CFG = mapping_ref.MapCfg()
VR, ZB, N = CFG.vision_range, CFG.z_bins, 120 * 160


def _obs(fr):
    return torch.from_numpy(mapping_scenes.frame_to_obs(fr))[None]


def _coords_feat(fr):
    obs = _obs(fr)
    coords = mapping_ref.point_cloud_std(obs[:, 3], CFG)
    feat = torch.ones(1, 11, N)
    feat[:, 1:] = obs[:, 4:].reshape(1, 10, -1)
    return coords, feat


def _my_z(fr):
    z = _coords_feat(fr)[0][0, 2]
    return z[(z > -1) & (z < 1)] * 2 + 1.6


def _forward(fr, start=mapping_scenes.CENTRE, maps=None, force=None):
    """Oracle forward of one frame; ``force`` = True / False overrides the decision of the stairs rule (what a kernel that
    decides wrongly would compute)."""
    orig = mapping_ref.stairs_mask
    if force is not None:
        def forced(coords, feat):
            z = coords[0, 2, :]
            return ((z * 2 + 1.6 < 0.7) & (feat[0, 1 + 4] == 0)) if force else torch.zeros_like(z, dtype=torch.bool)
        mapping_ref.stairs_mask = forced
    try:
        maps = torch.zeros(14, 480, 480) if maps is None else maps
        fp, mp, _, pose = mapping_ref.forward(_obs(fr), torch.from_numpy(fr["pose"]), maps, torch.tensor(start), CFG)
    finally:
        mapping_ref.stairs_mask = orig
    return fp, mp, pose


def _positions(fr):
    """Splat positions [3, N] (x, y, z in cells) after the stairs mask, as splat_feat_nd computes them."""
    coords, feat = _coords_feat(fr)
    coords[:, :, mapping_ref.stairs_mask(coords, feat)] = 99999
    dims = torch.tensor([VR, VR, ZB], dtype=torch.float32)[:, None]
    return (coords[0] * dims / 2 + dims / 2), feat


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "mapping_golden_edges.npz"))


PAIRS = {p["name"]: p for p in mapping_scenes.stairs_pairs()}


def test_height_frame_sets_my_z_pixel_by_pixel():
    heights = np.full((120, 160), np.nan)
    heights[60:, 10:150] = np.linspace(-30.0, 85.0, 140)[None, :]
    heights[:59, 10:150] = np.linspace(95.0, 350.0, 140)[None, :]
    fr = mapping_scenes._frame(mapping_scenes.height_frame(heights))
    z = _coords_feat(fr)[0][0, 2].reshape(120, 160)
    used = ~np.isnan(heights)
    my = (z * 2 + 1.6).numpy()
    assert np.abs(my[used] - heights[used] / 100.0).max() < 2e-6          # fp32 rounding of a value below 4
    assert not bool(((z > -1) & (z < 1))[torch.from_numpy(~used)].any())  # unused pixels: out of range on every row
    far = _coords_feat(mapping_scenes.far_frame())[0][0, 2].reshape(120, 160)
    assert bool(((far[59] > -1) & (far[59] < 1)).all())                   # ... which FAR_CM does not achieve on row 59


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_stairs_pair_is_on_both_sides_of_the_rule(name, golden):
    p = PAIRS[name]
    fps = []
    for k, side in enumerate("ab"):
        fr = p[side]
        my = _my_z(fr)
        n, le, mid = len(my), int((my <= 0.2).sum()), int(((my > 0.2) & (my < 0.7)).sum())
        assert (n, le, mid) == (p["n"][k], p["le"][k], p["mid"][k]), f"{name} {side}: n, le, mid = {n}, {le}, {mid}"
        coords, feat = _coords_feat(fr)
        mask = mapping_ref.stairs_mask(coords, feat)
        assert bool(mask.any()) == p["taken"][k] == bool(golden[f"stairs_{name}_{side}/stairs_branch"][0])
        ranks = np.float32(0.03) * np.float32(n - 1)
        k_lo, k_hi = int(ranks), int(math.ceil(ranks))
        q = float(torch.quantile(my, 0.03))
        if name == "interp":
            assert (n, k_lo, k_hi, le) == (1000, 29, 30, k_lo + 1) and abs(q - 0.2) >= 2e-3
            srt = torch.sort(my)[0]
            assert float(srt[k_lo]) <= 0.2 < float(srt[k_hi]) and (q > 0.2) == p["taken"][k]     # only the lerp decides
        if name == "le_sides":
            assert (k_lo, k_hi) == (29, 30) and le == (k_lo if k == 0 else k_hi + 1)
        if name == "mid_200":
            assert q > 0.2 and float(np.float32(0.2 * n)) == 200.0 and mid == (200, 201)[k]
        if name == "n2":
            assert (k_lo, k_hi, le) == (0, 1, 1) and abs(q - 0.2) >= 2e-3
        if name == "n101":
            assert float(ranks) == 3.0 and k_lo == k_hi == 3 and le == (3, 4)[k]
        # a wrong decision on this frame is visible: in the map always, in fp_map_pred wherever a removed point can lie in
        # the agent-height band at all (n1 b: its only point is at or below 0.2)
        fp, mp, _ = _forward(fr)
        fp_w, mp_w, _ = _forward(fr, force=not p["taken"][k])
        assert not torch.equal(mp, mp_w), f"{name} {side}: the other decision gives the same map"
        if (name, side) != ("n1", "b"):
            assert not torch.equal(fp, fp_w), f"{name} {side}: the other decision gives the same fp_map_pred"
        assert np.array_equal(np.packbits(fp.numpy().astype(bool)), golden[f"stairs_{name}_{side}/fp_map_bits"][0])
        fps.append((fp, mp))
    assert not torch.equal(fps[0][1], fps[1][1])                 # the two frames give different maps ...
    assert name == "n1" or not torch.equal(fps[0][0], fps[1][0])          # ... and fp_map_pred (n1: one of them can show only in the map)
    assert p["taken"][0] != p["taken"][1]
    if name == "toilet":                      # the surviving points are the toilet pixels' (and the ones above the band)
        a = p["a"]
        bare = dict(a, sem=a["sem"].copy())
        bare["sem"][4] = 0
        assert int(a["sem"][4].sum()) == 100 and not torch.equal(_forward(bare)[0], fps[0][0])


def test_empty_stairs_frame_has_no_point_in_range(golden):
    fr = mapping_scenes.stairs_empty_frame()
    assert len(_my_z(fr)) == 0
    fp, mp, _ = _forward(fr)
    assert float(fp.abs().sum()) == 0.0 and float(mp.abs().sum()) == 0.0 and golden["stairs_n0/final_idx"].size == 0


def _splat_in_order(feat, pos, reverse):
    """oracle.mapping_ref.splat with the scatter_add_ replaced by NumPy's unbuffered add.at: float32 adds one point after
    the other, in point order or (``reverse``) in the opposite order.  Returns (final grid, the eight pre-round grids)."""
    dims = (VR, VR, ZB)
    grid = np.zeros((feat.shape[1], VR * VR * ZB), np.float32)
    pos_dim, wts_dim = [], []
    for d in range(3):
        p = pos[d][None, None, :]
        pd, wd = [], []
        for ix in (0, 1):
            p_ix = torch.floor(p) + ix
            safe = ((p_ix > 0) & (p_ix < dims[d])).type(p.dtype)
            pd.append(p_ix * safe)
            wd.append((1 - torch.abs(p - p_ix)) * safe)
        pos_dim.append(pd)
        wts_dim.append(wd)
    pre = []
    for corner in ((a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)):
        wts = torch.ones_like(wts_dim[0][0])
        index = torch.zeros_like(wts_dim[0][0])
        for d in range(3):
            index = index * dims[d] + pos_dim[d][corner[d]]
            wts = wts * wts_dim[d][corner[d]]
        idx = index.long().numpy().reshape(-1)
        contrib = (feat * wts)[0].numpy()
        if reverse:
            idx, contrib = idx[::-1], contrib[:, ::-1]
        for f in range(grid.shape[0]):
            np.add.at(grid[f], idx, contrib[f])
        pre.append(grid.copy())
        grid = np.round(grid)
    return grid, pre


@pytest.mark.parametrize("depth_cm,seed,most", [(55.0, 1, 64), (10.0, 3, 1000)])
def test_dense_frames_have_crowded_cells_whose_order_matters(depth_cm, seed, most):
    fr = mapping_scenes.dense_frame(depth_cm, seed)
    pos, feat = _positions(fr)
    fl = torch.floor(pos)
    ok = (fl[0] >= 0) & (fl[0] < VR) & (fl[1] >= 0) & (fl[1] < VR) & (fl[2] >= 0) & (fl[2] < ZB)
    key = ((fl[0] * VR + fl[1]) * ZB + fl[2])[ok].long()
    counts = torch.bincount(key)
    print(f"depth {depth_cm}: {int((counts > 0).sum())} cells, largest {int(counts.max())}")
    assert int(counts.max()) >= most
    assert set(np.unique(fr["sem"])) == {0, 1, 2}
    fwd, pre = _splat_in_order(feat, pos, reverse=False)
    # the point-order replay IS the reference's sum: same bits as scatter_add_ on the coordinates themselves
    coords, feat2 = _coords_feat(fr)
    coords[:, :, mapping_ref.stairs_mask(coords, feat2)] = 99999
    assert np.array_equal(fwd, mapping_ref.splat(feat2, coords, (VR, VR, ZB)).reshape(11, -1).numpy())
    assert any(bool((g != np.round(g)).any()) for g in pre)                 # a pre-round sum that is not an integer
    rev, pre_rev = _splat_in_order(feat, pos, reverse=True)
    assert any(not np.array_equal(a, b) for a, b in zip(pre, pre_rev))      # fp32: the order changes a pre-round sum
    flips = int((fwd != rev).sum())
    # (a rounded voxel changes only by chance here: order_frame is the scene built so that one does)
    print(f"depth {depth_cm}: reversed order changes {flips} voxel values after rounding")


def _window(grid):
    """The 14-channel egocentric window [C, y, x] of mapping.py:99-128 from a voxel grid [11, x * y * z]."""
    v = torch.from_numpy(grid).view(11, VR, VR, ZB).transpose(1, 2)
    agent, allh = v[..., CFG.min_z:CFG.max_z].sum(3).clone(), v.sum(3)
    for f in CFG.all_height_cats:
        agent[f] = allh[f]
    return torch.cat([torch.clamp(agent[:1] / 0.1, 0, 1), torch.clamp(allh[:1], 0, 1), torch.zeros(2, VR, VR),
                      torch.clamp(agent[1:] / 5.0, 0, 1)])


def test_order_frame_rounds_differently_in_another_order(golden):
    fr = mapping_scenes.order_frame()
    pos, feat = _positions(fr)
    fl = torch.floor(pos)
    inside = (fl[0] >= 0) & (fl[0] < VR) & (fl[1] >= 0) & (fl[1] < VR) & (fl[2] >= 0) & (fl[2] < ZB)
    assert int(inside.sum()) == 3841 and bool(inside[-1])                       # the large one is the last point
    assert {tuple(int(v) for v in fl[:, i]) for i in torch.nonzero(inside)[:, 0]} == {(50, 0, 25)}
    wts = ((pos[0] - fl[0]) * (pos[1] - fl[1]) * (1 - (pos[2] - fl[2])))[inside]     # weight for corner (1, 1, 0)
    small, big = wts[:-1].double(), float(wts[-1])
    print(f"small: max {float(small.max()):.3e}, sum {float(small.sum()):.4e}; large {big!r}")
    assert float(small.max()) < 2.0 ** -26 and 0.25 <= big <= 0.5              # each below half an ulp of the large one
    assert 0.5 * float(small.sum()) < 0.5 - big < 0.9 * float(small.sum())      # most, not all, of them must come first
    fwd, _ = _splat_in_order(feat, pos, reverse=False)
    rev, _ = _splat_in_order(feat, pos, reverse=True)
    x, y, z = mapping_scenes.ORDER_VOXEL
    v = (x * VR + y) * ZB + z
    assert fwd[0, v] == 1.0 and rev[0, v] == 0.0
    wf, wr = _window(fwd), _window(rev)
    assert [float(wf[c, y, x]) for c in (1, 4 + 2, 4 + 5)] == [1.0, pytest.approx(0.2), pytest.approx(0.2)]
    assert [tuple(int(i) for i in t) for t in torch.nonzero(wf != wr)] == [(c, y, x) for c in (1, 4 + 2, 4 + 5)]
    assert float(wr[:, y, x].abs().sum()) == 0.0 and float(wf[0].sum()) == 0.0  # (fp_map_pred is empty either way)
    # the reference's own result (through the golden file) is the point-order one: the cell shows in the map
    _, mp, _ = _forward(fr)
    assert float(mp[1].sum()) > 0.5 and golden["dense_order/final_idx"].size > 0
    assert float(golden["dense_order/channel_sums"][0][1]) == pytest.approx(float(mp[1].double().sum()), abs=1e-6)


def test_dense_sequence_revisits_the_same_cells_after_an_empty_frame():
    seq = mapping_scenes.dense_sequence()
    assert len(seq) == 5 and float(seq[1]["depth"].min()) == mapping_scenes.FAR_CM
    assert np.array_equal(seq[0]["depth"], seq[2]["depth"]) and not np.array_equal(seq[0]["sem"], seq[2]["sem"])
    assert all(not fr["pose"].any() for fr in seq)
    fl = torch.floor(_positions(seq[1])[0])
    assert not bool(((fl[0] >= 0) & (fl[0] < VR) & (fl[1] >= 0) & (fl[1] < VR) & (fl[2] >= 0) & (fl[2] < ZB)).any())


def test_limit_frames_touch_and_cross_every_face_of_the_grid():
    frames = dict(mapping_scenes.limit_frames())
    integral = False
    for d, (name, dim) in enumerate((("limit_x", VR), ("limit_y", VR), ("limit_z", ZB))):
        pos, _ = _positions(frames[name])
        other = [k for k in range(3) if k != d]
        # points whose two other coordinates are inside the grid: only dimension d decides
        inside = torch.ones(N, dtype=torch.bool)
        for k in other:
            lim = ZB if k == 2 else VR
            inside &= (pos[k] >= 1) & (pos[k] < lim - 1)
        fl = torch.floor(pos[d])[inside]
        seen = {int(v) for v in fl.unique() if -3 <= v <= dim + 2}
        print(name, sorted(seen))
        assert {-1, 0, dim - 1, dim} <= seen, f"{name}: floor indices {sorted(seen)}"
        integral |= bool(((pos[d] == torch.floor(pos[d])) & inside & (pos[d] >= 0) & (pos[d] <= dim)).any())
    assert integral
    py = _positions(frames["limit_y"])[0][1]
    assert bool((py == 99.0).any()) and bool((py == 100.0).any()) and bool((py == 0.0).any())


def _run(frames, start):
    maps, pose, out = torch.zeros(14, 480, 480), torch.tensor(start), []
    for fr in frames:
        before = pose.clone()
        _, maps, _, pose = mapping_ref.forward(_obs(fr), torch.from_numpy(fr["pose"]), maps, pose, CFG)
        out.append((before, pose.clone()))
    return maps, out


SCENES = {s["name"]: s for s in mapping_scenes.edge_scenes()}


def test_heading_starts_cross_the_wrap():
    for name, sign in (("pose_wrap_pos", 1.0), ("pose_wrap_neg", -1.0)):
        sc = SCENES[name]
        _, steps = _run(sc["frames"], sc["start"])
        heads = [float(sc["start"][2])] + [float(p[2]) for _, p in steps]
        crossed = [i for i in range(1, len(heads)) if heads[i - 1] * heads[i] < 0 and min(abs(heads[i - 1]), abs(heads[i])) > 179]
        print(name, heads)
        assert crossed and heads[0] * sign > 0 and heads[-1] * sign < 0
        if name == "pose_wrap_pos":
            assert crossed == [2] and sc["start"][2] == 179.0          # on the second frame
    for name, want in (("pose_head_p180", 180.0), ("pose_head_m180", -180.0)):
        sc = SCENES[name]
        assert sc["start"][2] == want and all(float(f["pose"][2]) == 0.0 for f in sc["frames"])
        _, steps = _run(sc["frames"], sc["start"])
        assert all(abs(float(p[2])) == 180.0 for _, p in steps)
    sc = SCENES["pose_full_turn"]
    assert abs(float(sc["frames"][0]["pose"][2]) - (2 * math.pi + 0.3)) < 1e-6
    _, steps = _run(sc["frames"][:1], sc["start"])
    assert abs(float(steps[0][1][2]) - math.degrees(0.3)) < 1e-3


BORDER_KINDS = {"sw_in": "cut", "sw_out": "none", "e_along": "cut", "e_out": "none", "s_along": "cut", "s_out": "none",
                "ne_in": "full", "ne_out": "none", "outside": "none", "far_outside": "none"}


def test_border_starts_cut_the_window():
    edge_hit = False
    for name, start, inward in mapping_scenes.BORDER_STARTS:
        sc = SCENES[f"border_{name}"]
        assert tuple(sc["start"]) == start and len(sc["frames"]) == 2
        maps, _ = _run(sc["frames"][:1], start)
        centre, _ = _run(sc["frames"][:1], (12.0, 12.0, start[2]))
        assert BORDER_KINDS[name] == inward                    # (the GPU test's table)
        nnz, full = int((maps[0] != 0).sum()), int((centre[0] != 0).sum())
        print(f"{name}: channel 0 nnz {nnz} of {full} at the centre")
        if inward == "cut":
            assert 0 < nnz < full, f"{name}: {nnz} of {full}"
        elif inward == "full":
            assert 0 < nnz == full, f"{name}: {nnz} of {full}"
        else:
            assert nnz == 0 and float(maps.abs().sum()) == 0.0, name
        edge_hit |= bool((maps[:, 0] != 0).any() or (maps[:, -1] != 0).any() or (maps[:, :, 0] != 0).any() or (maps[:, :, -1] != 0).any())
    assert edge_hit
    assert [k for _, _, k in mapping_scenes.BORDER_STARTS].count("cut") >= 3
    assert SCENES["border_outside"]["start"][0] < 0 and SCENES["border_outside"]["start"][1] > 24.0


def test_edge_golden_file_is_made_from_these_scenes(golden, golden_dir):
    """Depth, semantics, poses and start of every scene are the builders' (the goldens cannot drift from the scenes the CPU
    tests above vouch for); depth is quantised to 1/4 cm except where a stairs frame needs its exact heights; < 1 MB."""
    assert os.path.getsize(os.path.join(golden_dir, "mapping_golden_edges.npz")) < 1_000_000
    assert {k.split("/")[0] for k in golden.files} == set(SCENES)
    for name, sc in SCENES.items():
        src = sc["source"] or name
        assert (f"{name}/source" in golden.files) == (sc["source"] is not None)
        if sc["source"] is not None:
            assert str(golden[f"{name}/source"]) == sc["source"]
        assert np.array_equal(golden[f"{src}/depth"][:len(sc["frames"])], np.stack([f["depth"] for f in sc["frames"]]))
        assert np.array_equal(golden[f"{src}/sem"][:len(sc["frames"])], np.stack([f["sem"] for f in sc["frames"]]))
        assert np.array_equal(golden[f"{name}/pose_obs"], np.stack([f["pose"] for f in sc["frames"]]))
        assert np.array_equal(golden[f"{name}/start"], np.asarray(sc["start"], np.float32))
        if sc["source"] is None:
            assert bool(golden[f"{name}/depth_quantised"]) == (name == "stairs_n0" or not name.startswith(("stairs_", "limit_z", "dense_order")))
