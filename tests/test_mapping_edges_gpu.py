"""The HIP map projection at its edges, against tests/golden/mapping_golden_edges.npz (the reference's own Semantic_Mapping on
oracle.mapping_scenes.edge_scenes(); oracle/gen_golden_mapping.py --edges) and, where no golden is stored (a random previous
map), against oracle.mapping_ref.forward.  tests/test_mapping_scenes_cpu.py proves on the CPU that every scene meets the
condition it is named after, so each test here fails under the matching mistake in peanut_amd/csrc/mapping.hip:

  stairs pairs   two frames one pixel or one count apart, on either side of mapping.py:94: the interpolated quantile
                 (le = k_lo + 1), le = k_lo / k_hi + 1, mid = 0.2 n at equality, n = 1, 2, 101 (integral rank), 0,
                 'toilet' pixels inside the removed band
  dense cells    81 and 2352 points in one cell, the same cells again after an empty frame, and a cell whose rounded sum
                 is 1 in point order and 0 once the large term comes before the small ones (dense_order)
  grid limits    floor cells 0 and dim - 1, one cell outside on either side of x, y and z, integral positions
  heading wrap   179 -> -179.6, -179.5 -> 179.8, +-180 held, a turn of 2 pi + 0.3
  border starts  the warped window cut by the border of the local map, and wholly outside it

Gates are the project's own (tests/test_mapping_gpu.py): fp_map_pred bit-equal, channel sums 0.05, poses 1e-5, map values
VAL_TOL = 3.5e-5; the wrapped heading is asserted bit-equal (plain fp32 arithmetic, contraction off on both sides).
NaN or negative values in maps_last are not tested: fmaxf and torch.max differ on NaN, and the reference never produces them.

Measured on an MI355X (max-abs of the final map against the golden / of every frame against the oracle):
  0 on every stairs, dense, limit and border scene and on wrap_pos, head_p180, head_m180, full_turn;
  2.5e-5 on wrap_neg (final map, golden); 1.9e-5 on border ne_in with a random previous map (heading -135), 0 on the other
  border starts with it.  The headings are bit-equal everywhere; no cell beyond a cut window was written.
"""
import os

import numpy as np
import pytest
import torch

from test_mapping_batch_gpu import _args, _batched_run, _module, _single_runs
from test_mapping_gpu import VAL_TOL

pytestmark = pytest.mark.gpu

assert VAL_TOL == 3.5e-5
POSE_TOL = 1e-5

STAIRS = ["interp", "le_sides", "mid_200", "n1", "n2", "n101", "toilet"]
LIMITS = ["limit_x", "limit_y", "limit_z"]
HEADINGS = ["wrap_pos", "wrap_neg", "head_p180", "head_m180", "full_turn"]
BORDERS = [("sw_in", "cut"), ("sw_out", "none"), ("e_along", "cut"), ("e_out", "none"), ("s_along", "cut"), ("s_out", "none"),
           ("ne_in", "full"), ("ne_out", "none"), ("outside", "none"), ("far_outside", "none")]


@pytest.fixture(scope="module")
def z(golden_dir):
    return np.load(os.path.join(golden_dir, "mapping_golden_edges.npz"))


@pytest.fixture(scope="module")
def sm():
    return _module(_args())


def _scene(z, name):
    """(obs [n,14,120,160], pose_obs [n,3], start [3]) of a golden scene; a scene with a source reuses its images."""
    src = str(z[f"{name}/source"]) if f"{name}/source" in z.files else name
    rel = z[f"{name}/pose_obs"]
    n = rel.shape[0]
    obs = np.zeros((n, 14, 120, 160), np.float32)
    obs[:, 3] = z[f"{src}/depth"][:n]
    obs[:, 4:] = z[f"{src}/sem"][:n].astype(np.float32)
    return torch.from_numpy(obs), torch.from_numpy(rel), torch.from_numpy(z[f"{name}/start"])


def _final(z, name):
    ref = np.zeros(14 * 480 * 480, np.float32)
    ref[z[f"{name}/final_idx"]] = z[f"{name}/final_val"]
    return ref


def _run_against_golden(sm, z, name, exact_heading=False):
    """Every frame of the scene from an empty map: fp_map_pred bits, pose and channel sums after every frame, the final map
    to VAL_TOL.  Returns per frame (fp_map_pred, map) on the host."""
    obs, rel, start = _scene(z, name)
    maps, pose, rec = torch.zeros(14, 480, 480, device="cuda"), start.cuda(), []
    for i in range(obs.shape[0]):
        fp, maps, _, _ = sm(obs[i:i + 1].cuda(), rel[i].cuda(), maps, pose, None)
        fp_h, m_h, p_h = fp.cpu(), maps.cpu(), pose.cpu().numpy()
        assert np.array_equal(np.packbits(fp_h.numpy().astype(bool)), z[f"{name}/fp_map_bits"][i]), f"{name} frame {i}: fp_map_pred"
        assert set(np.unique(fp_h.numpy())) <= {0.0, 1.0}
        want = z[f"{name}/poses"][i]
        assert np.abs(p_h - want).max() <= POSE_TOL, f"{name} frame {i}: pose {p_h} against {want}"
        if exact_heading:
            assert p_h[2] == want[2], f"{name} frame {i}: heading {p_h[2]!r} against {want[2]!r}"
        sums = m_h.numpy().astype(np.float64).sum((1, 2))
        np.testing.assert_allclose(sums, z[f"{name}/channel_sums"][i], rtol=0, atol=0.05, err_msg=f"{name} frame {i}: channel sums")
        rec.append((fp_h, m_h))
    err = float(np.abs(rec[-1][1].numpy().reshape(-1) - _final(z, name)).max())
    print(f"{name}: final map max-abs against the golden {err:.3e}")
    assert err <= VAL_TOL, f"{name}: final map max-abs {err:.3e}"
    return rec


@pytest.mark.parametrize("name", STAIRS)
def test_stairs_pairs(sm, z, name):
    a = _run_against_golden(sm, z, f"stairs_{name}_a")[0]
    b = _run_against_golden(sm, z, f"stairs_{name}_b")[0]
    assert bool(z[f"stairs_{name}_a/stairs_branch"][0]) != bool(z[f"stairs_{name}_b/stairs_branch"][0])
    assert not torch.equal(a[1], b[1]), f"{name}: both frames give the same map"
    if name != "n1":          # (its frame b has one point, at or below 0.2: outside the agent-height band either way)
        assert not torch.equal(a[0], b[0]), f"{name}: both frames give the same fp_map_pred"


def test_stairs_frame_without_a_point_in_range(sm, z):
    fp, maps = _run_against_golden(sm, z, "stairs_n0")[0]
    assert float(fp.abs().sum()) == 0.0 and float(maps.abs().sum()) == 0.0


def test_dense_sequence_frame_by_frame(sm, z):
    """dense (55 cm) -> all-far -> the same cells with other semantics -> 10 cm (2352 points in a cell) -> an ordinary frame."""
    rec = _run_against_golden(sm, z, "dense_seq")
    assert len(rec) == 5
    assert float(rec[1][0].abs().sum()) == 0.0 and torch.equal(rec[1][1], rec[0][1])      # the far frame adds nothing
    assert not torch.equal(rec[2][1], rec[1][1])


def test_dense_cell_is_summed_in_point_order(sm, z):
    """dense_order: explored area (and the two all-height categories) of one cell exist only if the 3840 small terms of its
    voxel are added before the large one, as scatter_add_ does; the channel sums would miss 1.0 (0.2, 0.2)."""
    fp, maps = _run_against_golden(sm, z, "dense_order")[0]
    assert float(fp.abs().sum()) == 0.0
    want = z["dense_order/channel_sums"][0]
    assert want[1] > 1.5 and want[4 + 2] > 0.3 and want[4 + 5] > 0.3


@pytest.mark.parametrize("name", LIMITS)
def test_grid_limits(sm, z, name):
    _run_against_golden(sm, z, name)


@pytest.mark.parametrize("name", HEADINGS)
def test_heading_wrap(sm, z, name):
    _run_against_golden(sm, z, f"pose_{name}", exact_heading=True)
    heads = [float(z[f"pose_{name}/start"][2])] + [float(p[2]) for p in z[f"pose_{name}/poses"]]
    if name.startswith("wrap"):
        assert min(heads) < -178.0 and max(heads) > 178.0


@pytest.mark.parametrize("name,kind", BORDERS)
def test_border_starts(sm, z, name, kind):
    """From an empty map against the golden; then on a random non-negative previous map against the oracle, frame by frame
    on the same previous map: values to VAL_TOL, and every cell the oracle leaves as it was has the previous map's bits on
    the device too -- nothing is written beyond the cut window (the whole map for the starts whose window misses it)."""
    from oracle import mapping_ref
    cfg = mapping_ref.MapCfg()
    rec = _run_against_golden(sm, z, f"border_{name}")
    assert (float(rec[-1][1].abs().sum()) == 0.0) == (kind == "none")
    obs, rel, start = _scene(z, f"border_{name}")
    last = torch.rand(14, 480, 480, generator=torch.Generator().manual_seed(7))
    pose_c, pose_g, worst = start.clone(), start.cuda(), 0.0
    for i in range(obs.shape[0]):
        _, out_c, _, pose_c = mapping_ref.forward(obs[i:i + 1], rel[i], last, pose_c, cfg)
        _, out_g, _, _ = sm(obs[i:i + 1].cuda(), rel[i].cuda(), last.cuda(), pose_g, None)
        out_g = out_g.cpu()
        worst = max(worst, float((out_g - out_c).abs().max()))
        kept = out_c == last
        assert torch.equal(out_g[kept], last[kept]), f"{name} frame {i}: {int((out_g[kept] != last[kept]).sum())} cells written beyond the window"
        if kind == "none":
            assert bool(kept.all()) and torch.equal(out_g, last)
        else:
            assert not bool(kept.all())
        assert float((pose_g.cpu() - pose_c).abs().max()) <= POSE_TOL
        last = out_c
    print(f"border_{name}: max-abs against the oracle on a random previous map {worst:.3e}")
    assert worst <= VAL_TOL, f"{name}: max-abs {worst:.3e} on a random previous map"


def test_edges_in_one_batch(z):
    """E = 4 in lock-step: stairs frames (taken, not taken, taken), dense cells around an empty frame, a start in the corner
    of the map and the heading wrap -- every slot has the bits of its single-episode run after every frame."""
    def cat(parts):
        obs, rel = zip(*[(_scene(z, n)[0][i], _scene(z, n)[1][i]) for n, i in parts])
        return torch.stack(obs).cuda(), torch.stack(rel).cuda()
    episodes = [cat([("stairs_interp_a", 0), ("stairs_interp_b", 0), ("stairs_mid_200_b", 0)]),
                cat([("dense_seq", 0), ("dense_seq", 1), ("dense_seq", 3)]),
                cat([("border_sw_in", 0), ("border_sw_in", 1), ("border_sw_in", 0)]),
                cat([("pose_wrap_pos", 0), ("pose_wrap_pos", 1), ("pose_wrap_pos", 2)])]
    starts = [(torch.zeros(14, 480, 480, device="cuda"), _scene(z, n)[2].cuda())
              for n in ("stairs_interp_a", "dense_seq", "border_sw_in", "pose_wrap_pos")]
    args = _args()
    want = _single_runs(args, episodes, starts)
    assert float(want[0][0][0].sum()) != float(want[0][1][0].sum())            # the stairs slot did change sides
    assert float(want[3][0][2][2]) > 179.0 and float(want[3][1][2][2]) < -179.0    # and the heading did wrap
    _batched_run(_module(args, reserve=4), episodes, starts, want)
