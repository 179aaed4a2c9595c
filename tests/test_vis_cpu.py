"""The visualisation frame without a device: the ABI, the two colour tables against PIL and matplotlib, the fixture and what its
cases claim to contain (checked on the golden arrays the reference's own ``_visualize`` produced), the argument checks."""
import ctypes as C
import os
import types

import numpy as np
import pytest

import vis_cases as vc
from peanut_amd import _lib
from peanut_amd import vis as pv


@pytest.fixture(scope="module")
def golden():
    return np.load(vc.GOLDEN)


@pytest.fixture(scope="module")
def cases():
    return {c["name"]: c for c in vc.golden_cases()}


def test_abi_and_symbols():
    lib = _lib.load()
    assert _lib.ABI_VERSION >= 23 and lib.peanut_abi_version() == _lib.ABI_VERSION
    for name in ("peanut_vis_index_map", "peanut_vis_render", "peanut_vis_render_batch", "peanut_vis_sem_argmax", "peanut_goal_fields"):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.VIS_FRAME_BYTES == _lib.VIS_H * _lib.VIS_W * 3 == 2547000 and _lib.VIS_FRAME_BYTES % 8 == 0


def test_palette_lut_is_what_pil_gives():
    """``putpalette(color_pal)`` / ``putdata`` / ``convert("RGB")`` (agent_helper.py:545-550) for all 256 indices."""
    from PIL import Image
    img = Image.new("P", (256, 1))
    img.putpalette([int(v) for v in pv._PALETTE_RGB])
    img.putdata(np.arange(256, dtype=np.uint8))
    got = np.asarray(img.convert("RGB"))[0]
    lut = pv.palette_lut()
    assert lut.shape == (256, 3) and lut.dtype == np.uint8
    assert np.array_equal(got, lut)
    assert not lut[24:].any() and len(pv._PALETTE_RGB) == 72
    assert pv.arrow_colour() == (int(lut[3, 2]), int(lut[3, 1]), int(lut[3, 0]))      # palette entries 11, 10, 9


def test_purples_table_is_what_matplotlib_gives():
    table = pv.purples_bgr()
    assert table.shape == (257, 3) and table.dtype == np.uint8 and not table[256].any()
    matplotlib = pytest.importorskip("matplotlib")
    cm = matplotlib.colormaps["Purples"]
    assert cm.N == 256
    want = np.array([(np.array(cm(i))[[2, 1, 0]] * 255).astype(np.uint8) for i in range(256)], np.uint8)
    assert np.array_equal(table[:256], want)
    # the call the reference makes: floats through `xa *= N`, NaN to the bad colour
    x = np.array([0.0, 1.0, 0.5, 3 / 256, np.nextafter(1.0, 0.0), np.nan])
    ref = (cm(x)[:, [2, 1, 0]] * 255).astype(np.uint8)
    assert np.array_equal(ref, table[vc.colour_index(np.array([0.0, 1.0, 0.5, 3 / 256, np.nextafter(1.0, 0.0)])).tolist() + [256]])
    # several entries truncate one below what k / 255 * 255 rounds to: the table cannot be recomputed from rounded bytes
    rounded = np.array([np.round(np.array(cm(i))[[2, 1, 0]] * 255) for i in range(256)])
    assert (rounded != want).any()


def test_fixture_size_and_contents(golden, cases):
    size = os.path.getsize(vc.GOLDEN)
    assert size < 1536 * 1024 and size < 1024 * 1024, size
    for name, c in cases.items():
        assert golden[f"{name}/index"].shape == (c["m"], c["m"]) and golden[f"{name}/index"].dtype == np.uint8
        assert golden[f"{name}/frame"].shape == (600, 1415, 3) and golden[f"{name}/frame"].dtype == np.uint8
        assert golden[f"{name}/arrow"].shape == (4, 2)
    assert all(v.dtype.kind in "iu" for v in golden.values())
    claimed = {cl for c in cases.values() for cl in c["claims"]}
    assert claimed >= set(vc.REQUIRED_CLAIMS), set(vc.REQUIRED_CLAIMS) - claimed
    assert {c["m"] for c in cases.values()} == {480, 240, 96, 8, 1} and {c["ncat"] for c in cases.values()} == {10, 16, 22}
    c = cases["m480_view"]
    assert c["full"] == 960 and c["lmb"][0] > 0 and c["lmb"][2] > 0          # a strided view into the full map


def _window(c, a):
    gx1, gx2, gy1, gy2 = c["lmb"]
    return a[..., gx1:gx2, gy1:gy2]


def _check_claim(claim, c, idx, frame):
    from scipy import ndimage as ndi
    m, ncat = c["m"], c["ncat"]
    lm = _window(c, c["full_map"])
    col, visd = _window(c, c["collision"]) == 1, _window(c, c["visited"]) == 1
    dil = ndi.binary_dilation(c["goal"] != 0, structure=vc.disk(4))
    plain = ~visd & ~dil
    stg = None if c["stg"] is None else (int(c["stg"][0]), int(c["stg"][1]))
    if stg is not None and stg[0] < m and stg[1] < m:
        plain[stg] = False
    if claim == "collapse14":
        assert ncat == 10 and (col & plain).any() and not (idx == 14).any()
        assert np.isin(idx[col & plain], (0, 1, 2)).all()
        want = np.where(np.rint(lm[0]) == 1, 1, np.where(np.rint(lm[1]) == 1, 2, 0))
        assert np.array_equal(idx[col & plain], want[col & plain])
    elif claim == "no_collapse14":
        assert ncat != 10 and (col & plain).any() and (idx[col & plain] == 14).all()
    elif claim == "stg_skipped":
        assert stg is not None and (stg[0] >= m or stg[1] >= m) and np.array_equal(idx, vc.index_map(dict(c, stg=None)))
    elif claim == "stg_wraps":
        assert min(stg) < 0 and idx[stg[0] % m, stg[1] % m] == 15
        assert np.argwhere(idx != vc.index_map(dict(c, stg=None))).tolist() == [[stg[0] % m, stg[1] % m]]
    elif claim == "goal_borders":
        g = c["goal"] != 0
        assert g[0, 0] and g[0, 1:-1].any() and g[-1, 1:-1].any() and g[1:-1, 0].any() and g[1:-1, -1].any()
        assert np.array_equal(idx == 4, dil)
        assert (idx[:5, :5] == 4).sum() == int(vc.disk(4)[4:, 4:].sum())       # the corner keeps a quarter of the disk
    elif claim == "all_zero":
        zero = ~lm[4:4 + ncat - 1].any(axis=0) & plain & ~col
        assert zero.any() and np.isin(idx[zero], (0, 1, 2)).all()
        for v, mask in ((1, np.rint(lm[0]) == 1), (2, (np.rint(lm[1]) == 1) & (np.rint(lm[0]) != 1))):
            assert (zero & mask).any() and (idx[zero & mask] == v).all()
        assert (idx[zero & (np.rint(lm[0]) != 1) & (np.rint(lm[1]) != 1)] == 0).all()
    elif claim == "tie_1e5":
        r, q = c["tie_cell"]
        assert lm[4 + 2, r, q] == np.float32(1e-5) and not np.delete(lm[4:4 + ncat - 1, r, q], 2).any() and idx[r, q] == 2 + 5
        r, q = c["tie13_cell"]
        assert lm[4 + 1, r, q] == lm[4 + 3, r, q] == lm[4:4 + ncat - 1, r, q].max() and idx[r, q] == 1 + 5
    elif claim == "visited_over_goal":
        assert visd[m // 2 + 2, m // 2 + 2] and idx[m // 2 + 2, m // 2 + 2] == 4
        assert visd[m // 2 + 9, m // 2] and idx[m // 2 + 9, m // 2] == 3
    elif claim == "normed_0_1":
        for f in (c["target_pred"], c["value"], c["dd_wt"]):
            normed = (f - f.min()) / (f.max() - f.min())
            assert (normed == 0).any() and (normed == 1).any()
            assert set(vc.colour_index(f)[normed == 1].tolist()) == {255}
    elif claim == "integer_scaled":
        f = c["target_pred"]
        scaled = (f - f.min()) / (f.max() - f.min()) * f.dtype.type(256)
        assert ((scaled == np.floor(scaled)) & (scaled > 0) & (scaled < 256)).any()
    elif claim == "beyond_palette":
        assert idx.max() >= 24
        i, j = np.argwhere(idx >= 24)[0]
        y, x = 50 + (m - 1 - i) * (480 // m), 670 + j * (480 // m)
        assert not frame[y, x].any()                                           # PIL pads the palette with zeros: black
    elif claim == "no_pred":
        assert c["target_pred"] is None and (frame[40:540, 1165:] == 255).all()
    elif claim == "rgb_none":
        assert c["rgb"] is None and (frame[50:530, 15:655] == 255).all()
    elif claim == "black_dd_wt":
        assert not frame[50:290, 1165:1405].any() and (frame[49, 1165:1405] == 100).all()
    elif claim == "black_value":
        assert not frame[290:530, 1165:1405].any()
    elif claim == "float_differs":
        # float32 storage normalised in float (the reference's path when the prediction window is the whole map): neither extreme
        # is 0 and the span is no power of two, and the frame in double arithmetic is ANOTHER frame -- the golden is the float one
        tp = c["target_pred"]
        assert tp.dtype == np.float32 and c["bits"] == 32 and m >= 96 and tp.min() != 0
        span = float(tp.max() - tp.min())
        assert np.log2(span) != np.floor(np.log2(span))
        assert (vc.colour_index(tp) != vc.colour_index(tp.astype(np.float64))).sum() >= 8
        bg = pv.init_vis_image(c["goal_name"], vc.legend())
        as_float = vc.restate(c, bg, pv.palette_lut(), pv.purples_bgr())
        as_double = vc.restate(dict(c, target_pred=tp.astype(np.float64)), bg, pv.palette_lut(), pv.purples_bgr())
        assert np.array_equal(as_float, frame)
        assert (as_float != as_double).any(axis=2).sum() >= 8 * 25        # eight cells of 5 x 5 pixels at the least
    elif claim == "small":
        assert m < 9
    else:
        raise AssertionError(f"unknown claim {claim}")


def test_every_case_contains_what_it_claims(golden, cases):
    for name, c in cases.items():
        for claim in c["claims"]:
            try:
                _check_claim(claim, c, golden[f"{name}/index"].astype(np.int64), golden[f"{name}/frame"])
            except AssertionError as e:
                raise AssertionError(f"{name}: claim {claim}: {e}") from e


def test_restatement_matches_the_golden_frames(golden, cases):
    """The restatement the unpinned tests lean on gives the reference's frames (small cases; the generator checks all)."""
    for name in ("m96_x5", "m96_nan", "m8", "m1"):
        c = cases[name]
        bg = pv.init_vis_image(c["goal_name"], vc.legend())
        assert np.array_equal(vc.index_map(c), golden[f"{name}/index"])
        assert np.array_equal(vc.restate(c, bg, pv.palette_lut(), pv.purples_bgr()), golden[f"{name}/frame"])


def test_host_side_against_the_reference(golden, cases):
    """The arrow's vertices and colour and the file name, formed on the host."""
    for name, c in cases.items():
        pose = np.array([*c["pose"], *c["lmb"]], np.float64)
        assert np.array_equal(pv.contour_points(pv.arrow_pos(pose, c["m"], vc.RES)), golden[f"{name}/arrow"])
        assert pv.arrow_colour() == tuple(golden[f"{name}/colour"].tolist())
        args = types.SimpleNamespace(dump_location="D", exp_name="exp")
        assert pv.frame_path(args, c["rank"], c["episode_no"], c["timestep"])[1] == bytes(golden[f"{name}/fname"]).decode()


def test_fill_polygon_restatement():
    tri = vc.fill_polygon([(2, 2), (6, 2), (2, 6), (2, 6)], shape=(10, 10))
    want = np.zeros((10, 10), bool)
    for y in range(2, 7):
        want[y, 2:2 + (7 - y)] = True                                          # x + y <= 8, edges included
    assert np.array_equal(tri, want)
    assert vc.fill_polygon([(3, 4)] * 4, shape=(10, 10)).sum() == 1
    assert np.array_equal(np.argwhere(vc.fill_polygon([(1, 1), (4, 1), (6, 1), (2, 1)], shape=(10, 10))), [[1, x] for x in range(1, 7)])
    assert vc.fill_polygon([(-5, -5), (-2, -5), (-2, -2), (-5, -2)], shape=(10, 10)).sum() == 0


def test_nearest_index_rule():
    assert np.array_equal(vc.nearest_index(480, 480), np.arange(480))
    assert np.array_equal(vc.nearest_index(240, 480), np.arange(240) * 2)
    assert np.array_equal(vc.nearest_index(480, 96), np.arange(480) // 5)
    assert vc.nearest_index(480, 1).max() == 0 and vc.nearest_index(240, 100).max() == 99


def test_stg_resolution():
    assert pv.resolve_stg((3.9, 4.2), 8) == (3, 4) and pv.resolve_stg((-8, -1), 8) == (-8, -1) and pv.resolve_stg(None, 8) == (8, 8)
    assert pv.resolve_stg((8, -100), 8) == (8, -100)                          # skipped before it indexes (:520)
    with pytest.raises(ValueError):
        pv.resolve_stg((-9, 0), 8)
    with pytest.raises(ValueError):
        pv.resolve_stg((0, -9), 8)


def _structs(m=8, full=16):
    """Argument structs with made-up (never dereferenced) device addresses: every call below is refused before a launch."""
    cm = _lib.VisCommonC(m=m, channels=14, full_w=full, full_h=full, background=0x1000, palette=0x2000, cmap=0x3000, stream=None)
    ep = _lib.VisEpisodeC(local_map=0x10000, plane_stride=m * m, row_stride=m, collision_map=0x20000, visited_vis=0x30000, goal=0x40000,
                          index_map=0x50000, ranges=0x60000, frame=0x70000)
    ep.lmb[:] = [0, m, 0, m]
    ep.stg[:] = [m, m]
    return cm, ep


@pytest.mark.parametrize("what", ["null_local_map", "null_frame", "null_table", "m0", "row_overlap", "plane_overlap", "stg_low", "lmb_outside",
                                  "lmb_size", "misaligned_frame", "pred_without_value", "bits", "bits_below_data", "arrow_far"])
def test_refusals_enqueue_nothing(what):
    lib = _lib.load()
    cm, ep = _structs()
    if what == "null_local_map":
        ep.local_map = None
    elif what == "null_frame":
        ep.frame = None
    elif what == "null_table":
        cm.cmap = None
    elif what == "m0":
        cm.m = 0
    elif what == "row_overlap":
        ep.row_stride = 7
    elif what == "plane_overlap":
        ep.plane_stride = 63
    elif what == "stg_low":
        ep.stg[:] = [-9, 0]
    elif what == "lmb_outside":
        ep.lmb[:] = [9, 17, 0, 8]
    elif what == "lmb_size":
        ep.lmb[:] = [0, 7, 0, 8]
    elif what == "misaligned_frame":
        ep.frame = 0x70004
    elif what == "pred_without_value":
        ep.target_pred = 0x80000
        ep.bits[:] = [32, 64, 64]
        ep.data_bits[:] = [32, 64, 64]
    elif what in ("bits", "bits_below_data"):
        ep.target_pred, ep.value, ep.dd_wt = 0x80000, 0x90000, 0xa0000
        ep.bits[:] = [16, 64, 64] if what == "bits" else [32, 64, 64]
        ep.data_bits[:] = [32, 64, 64] if what == "bits" else [64, 64, 64]
    elif what == "arrow_far":
        ep.arrow[2][0] = 1 << 21
    assert lib.peanut_vis_render(C.byref(cm), C.byref(ep)) == -2          # PEANUT_EINVAL
    assert lib.peanut_last_error()


def test_batch_refusals_enqueue_nothing():
    lib = _lib.load()
    cm, ep = _structs()
    eps = (_lib.VisEpisodeC * 17)(*[ep] * 17)
    for E in (0, 17, -1):
        assert lib.peanut_vis_render_batch(C.byref(cm), E, eps) == -2
    assert lib.peanut_vis_render_batch(C.byref(cm), 2, eps) == -2             # two episodes name the same frame
    assert b"same output" in lib.peanut_last_error()
    assert lib.peanut_vis_render_batch(None, 1, eps) == -2 and lib.peanut_vis_render_batch(C.byref(cm), 1, None) == -2
    assert lib.peanut_vis_sem_argmax(C.byref(cm), None, 64, 8, 0x1000) == -2
    assert lib.peanut_vis_sem_argmax(C.byref(cm), 0x1000, 64, 7, 0x2000) == -2
    assert lib.peanut_vis_sem_argmax(None, 0x1000, 64, 8, 0x2000) == -2
    out = (C.c_void_p(), C.c_void_p(), (C.c_int * 2)())
    assert lib.peanut_goal_fields(None, C.byref(out[0]), C.byref(out[1]), C.byref(out[2])) == -2
