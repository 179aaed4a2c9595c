"""The device renderer of the visualisation frame (csrc/vis.hip, peanut_amd/vis.py), all bit for bit:

1. index map and frame against tests/golden/vis_golden.npz (the reference's own ``_visualize`` on tests/vis_cases.py); the arrow,
   which the fixture does not hold, painted into the expected frame by the restated fill rule from the reference's vertices;
2. the arrow alone against the restatement: at the panel's corners, partly outside the frame, with coinciding vertices;
3. m = 100 (inexact resize ratios) against the restated resize;
4. batches of 1, 3 and 16 mixed episodes equal to the single calls;
5. ``Agent_State.planner_inputs`` with and without ``args.visualize``; ``GeodesicSolver.fields``;
6. ``Agent_Helper.plan_act`` with ``visualize = 2`` on a chain of tests/plan_cases.py: the actions of the same chain without it, one
   decodable file per step."""
import os
import sys
import types
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import plan_cases as pc
import plan_world as pw
import vis_cases as vc
from peanut_amd import vis as pv

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = {c["name"]: c for c in vc.golden_cases()}


@pytest.fixture(scope="module")
def golden():
    return np.load(vc.GOLDEN)


_renderers = {}


def renderer(ncat):
    if ncat not in _renderers:
        _renderers[ncat] = pv.VisRenderer(SimpleNamespace(num_sem_categories=ncat, map_resolution=vc.RES), DEV, legend=vc.legend())
    return _renderers[ncat]


def item_of(c, **over):
    """A case on the device: the local map a view into the full map (strided unless the window is the whole map); a float64
    target_pred goes up as the fp32 it holds, with ``target_bits = 64`` (fp32 storage, double arithmetic)."""
    gx1, gx2, gy1, gy2 = c["lmb"]
    full_map = torch.from_numpy(c["full_map"]).to(DEV)
    it = dict(local_map=full_map[:, gx1:gx2, gy1:gy2], collision_map=torch.from_numpy(c["collision"]).to(DEV),
              visited_vis=torch.from_numpy(c["visited"]).to(DEV), lmb=c["lmb"], goal=torch.from_numpy(c["goal"]).to(DEV), stg=c["stg"],
              pose_pred=np.array([*c["pose"], *c["lmb"]], np.float64), goal_name=c["goal_name"],
              rgb=None if c["rgb"] is None else torch.from_numpy(c["rgb"]).to(DEV))
    if c["target_pred"] is not None:
        it.update(target_pred=torch.from_numpy(c["target_pred"].astype(np.float32)).to(DEV), value=torch.from_numpy(c["value"]).to(DEV),
                  dd_wt=torch.from_numpy(c["dd_wt"]).to(DEV), target_bits=c["bits"])
    it.update(over)
    return it


def with_arrow(frame, pts, colour):
    out = frame.copy()
    out[vc.fill_polygon(pts)] = colour
    return out


def differing(a, b):
    d = np.argwhere((a != b).any(axis=-1)) if a.ndim == 3 else np.argwhere(a != b)
    return f"{len(d)} differ, first at {d[:5].tolist()}"


@pytest.mark.parametrize("name", list(CASES))
def test_index_map_and_frame_equal_the_reference(name, golden):
    c = CASES[name]
    r = renderer(c["ncat"])
    it = item_of(c)
    if c["full"] > c["m"]:
        assert not it["local_map"].is_contiguous()
    idx = r.index_map(**it).cpu().numpy()
    assert np.array_equal(idx, golden[f"{name}/index"]), differing(idx, golden[f"{name}/index"])
    frame = r.render(**it)
    assert frame.shape == (600, 1415, 3) and frame.dtype == torch.uint8 and frame.is_cuda
    want = with_arrow(golden[f"{name}/frame"], golden[f"{name}/arrow"], pv.arrow_colour())
    got = r.frame_host()[0]
    assert np.array_equal(got, frame.cpu().numpy())
    assert np.array_equal(got, want), differing(got, want)
    assert np.array_equal(r._index[0].cpu().numpy(), golden[f"{name}/index"])
    # outside the arrow's pixels the frame is the reference's own
    clear = ~vc.fill_polygon(golden[f"{name}/arrow"])
    assert np.array_equal(got[clear], golden[f"{name}/frame"][clear])


def test_arithmetic_width_is_the_callers(golden):
    """The same fp32 prediction (m96_f32: min 0.3f, a span that is no power of two, values on both sides of the rounding of the
    float quotient) normalised in float and in double gives DIFFERENT frames; the float one is the reference's own (the fixture),
    each equals the restatement in that arithmetic; fp64 storage equals fp32 storage under double arithmetic."""
    c = CASES["m96_f32"]
    r = renderer(c["ncat"])
    bg = pv.init_vis_image(c["goal_name"], vc.legend())
    frames = {}
    for bits in (32, 64):
        tp = c["target_pred"].astype(np.float32 if bits == 32 else np.float64)
        want = vc.restate(dict(c, target_pred=tp), bg, pv.palette_lut(), pv.purples_bgr(), golden["m96_f32/arrow"], pv.arrow_colour())
        r.render(**item_of(c, target_bits=bits))
        frames[bits] = r.frame_host()[0].copy()
        assert np.array_equal(frames[bits], want), (bits, differing(frames[bits], want))
    assert np.array_equal(frames[32], with_arrow(golden["m96_f32/frame"], golden["m96_f32/arrow"], pv.arrow_colour()))
    assert (frames[32] != frames[64]).any(axis=2).sum() >= 8 * 25, "the two widths give one frame: the kernel ignores `bits`"
    r.render(**item_of(c, target_pred=torch.from_numpy(c["target_pred"].astype(np.float64)).to(DEV), target_bits=64))
    assert np.array_equal(r.frame_host()[0], frames[64])
    with pytest.raises(ValueError):
        r.render(**item_of(c, target_pred=torch.from_numpy(c["target_pred"].astype(np.float64)).to(DEV), target_bits=32))


@pytest.mark.parametrize("name,pts", vc.arrow_cases())
def test_arrow_fill_equals_the_restated_rule(name, pts, golden):
    c = CASES["m96_nopred"]
    r = renderer(c["ncat"])
    r.render(**item_of(c, arrow=pts))
    got = r.frame_host()[0]
    want = with_arrow(golden["m96_nopred/frame"], pts, pv.arrow_colour())
    assert np.array_equal(got, want), differing(got, want)
    if name == "outside":
        assert np.array_equal(got, golden["m96_nopred/frame"])
    if name == "panel_top_left":
        assert tuple(got[50, 670]) == pv.arrow_colour() and tuple(got[50, 682]) == pv.arrow_colour()


def test_inexact_resize_ratio_equals_the_restated_rule():
    c = vc.resize_case()
    r = renderer(c["ncat"])
    idx = r.index_map(**item_of(c)).cpu().numpy()
    assert np.array_equal(idx, vc.index_map(c))
    r.render(**item_of(c))
    pose = np.array([*c["pose"], *c["lmb"]], np.float64)
    want = vc.restate(c, pv.init_vis_image(c["goal_name"], vc.legend()), pv.palette_lut(), pv.purples_bgr(),
                      pv.contour_points(pv.arrow_pos(pose, c["m"], vc.RES)), pv.arrow_colour())
    got = r.frame_host()[0]
    assert np.array_equal(got, want), differing(got, want)
    assert sorted(set(np.bincount(vc.nearest_index(480, 100)).tolist())) == [4, 5]      # the ratio 4.8: runs of 4 and 5 pixels


def _mixed_items(E, two_names=False):
    """E episodes of one map size (m = 96, ncat = 10, the window the whole map): with and without a prediction, with and without rgb,
    constant and infinite fields, every stg and pose different; ``two_names``: every fourth episode has another goal name."""
    base = [CASES["m96_nopred"], CASES["m96_const"], CASES["m96_inf"]]
    items = []
    for e in range(E):
        c = base[e % 3]
        over = dict(stg=(e * 5 % 96, (e * 11 + 3) % 96), pose_pred=np.array([*vc.pose_at(96, (0, 0), 0.1 + 0.05 * e, 0.9 - 0.05 * e, 23.0 * e), *c["lmb"]]))
        if two_names and e % 4 == 3:
            over["goal_name"] = "bed"
        if e % 5 == 4:
            over["rgb"] = torch.from_numpy(vc.rgb_frame(e)).to(DEV)
        items.append(item_of(c, **over))
    return items


class _Calls:
    """Counts what ``render_batch`` hands to the library: (entry point, episodes) per call."""

    def __init__(self, monkeypatch):
        from peanut_amd import _lib
        lib = _lib.load()
        self.seen = []
        single, batch = lib.peanut_vis_render, lib.peanut_vis_render_batch

        def render(common, ep):
            self.seen.append(("peanut_vis_render", 1))
            return single(common, ep)

        def render_batch(common, E, eps):
            self.seen.append(("peanut_vis_render_batch", int(E)))
            return batch(common, E, eps)
        monkeypatch.setattr(lib, "peanut_vis_render", render)
        monkeypatch.setattr(lib, "peanut_vis_render_batch", render_batch)


@pytest.mark.parametrize("E,two_names", [(1, False), (3, False), (16, False), (16, True)])
def test_batches_equal_single_calls(E, two_names, monkeypatch):
    """One goal name: ONE library call with all E episodes (E = 16 fills every slot of the argument block and grid dimension).  Two
    goal names (two title bars): one call per name, 12 + 4."""
    items = _mixed_items(E, two_names)
    single = pv.VisRenderer(SimpleNamespace(num_sem_categories=10, map_resolution=vc.RES), DEV, legend=vc.legend())
    want = []
    for it in items:
        single.render(**it)
        want.append(single.frame_host()[0].copy())
    r = renderer(10)
    calls = _Calls(monkeypatch)
    frames = r.render_batch(items)
    if E == 1:
        assert calls.seen == [("peanut_vis_render", 1)]
    elif two_names:
        assert calls.seen == [("peanut_vis_render_batch", 12), ("peanut_vis_render_batch", 4)]
    else:
        assert calls.seen == [("peanut_vis_render_batch", E)]
    assert frames.shape == (E, 600, 1415, 3)
    got = r.frame_host()
    for e in range(E):
        assert np.array_equal(got[e], want[e]), (e, differing(got[e], want[e]))
    if E > 1:
        assert not np.array_equal(got[0], got[1])
        assert len({got[e].tobytes() for e in range(E)}) == E           # every slot rendered its own episode
    with pytest.raises(ValueError):
        r.render_batch([])
    with pytest.raises(ValueError):
        r.render_batch(items * 17)


def test_renderer_refuses_before_any_launch():
    c = CASES["m8"]
    r = renderer(10)
    r.render(**item_of(c))
    before = r.frame_host()[0].copy()
    for over in (dict(stg=(-9, 0)), dict(rgb=torch.zeros((480, 641, 3), dtype=torch.uint8, device=DEV)),
                 dict(rgb=torch.zeros((480, 640, 3), dtype=torch.float32, device=DEV)), dict(value=None),
                 dict(goal=torch.zeros((8, 9), dtype=torch.uint8, device=DEV))):
        with pytest.raises(ValueError):
            r.render(**item_of(c, **over))
    assert np.array_equal(r.frame_host()[0], before)


# ---- the host side ---------------------------------------------------------------------------------------------------------------
TODAYS_KEYS = {'obstacle', 'exp_pred', 'pose_pred', 'goal', 'found_goal', 'goal_name'}


def _state(**over):
    from peanut_amd.agent_state import Agent_State, default_args
    args = default_args(goal_map=True, **over)                       # the reference's geometry: 960 x 960, a 480 x 480 window
    st = Agent_State(args)
    st.reset()
    g = torch.Generator().manual_seed(5)
    lm = torch.rand(st.local_map.shape, generator=g)
    lm[4:, :20] = 0.0                                                 # no category anywhere in these rows
    st.local_map.copy_(lm)
    st.goal_map = torch.zeros((st.local_w, st.local_h), dtype=torch.uint8, device=st.device)
    return st


def test_planner_inputs_carry_sem_map_pred_only_with_visualize():
    infos = {'goal_name': 'chair'}
    plain = _state()
    assert set(plain.planner_inputs(infos)) == TODAYS_KEYS and set(plain.planner_inputs(infos, host=False)) == TODAYS_KEYS
    st = _state(visualize=1)
    p = st.planner_inputs(infos)
    assert set(p) == TODAYS_KEYS | {'sem_map_pred'}
    vlm = torch.clone(st.local_map[4:, :, :])                         # agent_state.py:259-262
    vlm[-1] = 1e-5
    want = vlm.argmax(0).cpu().numpy()
    assert p['sem_map_pred'].dtype == np.int64 and np.array_equal(p['sem_map_pred'], want)
    assert (want[:20] == st.nc - 5).all() and len(set(want[20:].ravel().tolist())) == st.nc - 5
    dev = st.planner_inputs(infos, host=False)
    assert set(dev) == TODAYS_KEYS | {'sem_map_pred'} and dev['sem_map_pred'] is st.local_map
    # a strided view (the local map inside the full map) gives the same
    full = torch.zeros((st.nc, 600, 640), device=st.device)
    full[:, 40:520, 50:530] = st.local_map
    assert torch.equal(pv.sem_argmax(full[:, 40:520, 50:530]).cpu(), torch.from_numpy(want).to(torch.uint8))


def test_goal_solver_fields_are_views_of_the_last_select():
    from peanut_amd.goal import GeodesicSolver
    from peanut_amd import _lib
    H = 64
    solver = GeodesicSolver(H, H, 2, device=DEV)
    with pytest.raises(_lib.PeanutHipError):
        solver.fields()
    obstacle = torch.zeros((H, H), device=DEV)
    obstacle[20, 5:50] = 1.0
    zeros = torch.zeros((H, H), dtype=torch.uint8, device=DEV)
    g = torch.Generator().manual_seed(3)
    tp = torch.rand((32, 32), generator=g).to(DEV)
    lmb = [16, 48, 16, 48]
    res = solver.select(obstacle, zeros, zeros, lmb, (30, 30), tp, 500.0, 5, want_value=True)
    dd_wt, value = solver.fields()
    assert dd_wt.shape == value.shape == (32, 32) and dd_wt.dtype == value.dtype == torch.float64 and dd_wt.is_cuda
    assert torch.equal(tp.double() * dd_wt, res["value"])             # value = target_pred * dd_wt (:407)
    res2 = solver.select(obstacle, zeros, zeros, lmb, (30, 30), tp, 500.0, 5)
    dd_wt2, value2 = solver.fields()
    assert dd_wt2.data_ptr() == dd_wt.data_ptr()                      # views, not copies
    assert torch.equal(value2, res["value"]) and float(value2.max()) == res2["value_max"]
    assert float(dd_wt2.max()) <= 1.0 and float(dd_wt2.min()) >= 0.0


def test_agent_state_keeps_the_solver_fields_only_with_visualize():
    """``update_global_goal`` on a real ``Agent_State``: with ``args.visualize`` it keeps ``dd_wt`` / ``value`` (the solver's own
    buffers), ``reset`` forgets them with ``target_pred``, ``vis_item`` hands them on with the arithmetic ``prediction_window``
    implies, and the frame rendered from that item equals the one rendered from copies of the fields."""
    def select(st):
        g = torch.Generator().manual_seed(9)
        st.full_map[0, 470:473, 300:700] = 1.0                       # a wall the field has to go round
        st.loc_r, st.loc_c = 480, 480
        st.target_pred = torch.rand((st.local_w, st.local_h), generator=g).to(st.device)
        st.update_global_goal()
    plain = _state()
    select(plain)
    assert plain.dd_wt is None and plain.value is None
    st = _state(visualize=1)
    select(st)
    assert st.dd_wt.shape == st.value.shape == (480, 480) and st.dd_wt.dtype == st.value.dtype == torch.float64
    assert torch.equal(st.value, st.target_pred.double() * st.dd_wt)                      # :407
    assert float(st.value.max()) == st.value_max == plain.value_max
    assert list(st.global_goals) == list(plain.global_goals)
    solver_dd, solver_value = st._goal_solver().fields()
    assert st.dd_wt.data_ptr() == solver_dd.data_ptr() and st.value.data_ptr() == solver_value.data_ptr()
    p = st.planner_inputs({'goal_name': 'chair'}, host=False)
    item = st.vis_item(p, stg=(200.0, 210.0))
    assert item["target_bits"] == 64 and item["value"] is st.value and item["dd_wt"] is st.dd_wt and item["target_pred"] is st.target_pred
    st.args.prediction_window = st.full_w                            # the window is the whole map: the reference stays in float32
    assert st.vis_item(p)["target_bits"] == 32
    st.args.prediction_window = 720
    r = renderer(10)
    r.render(**item)
    from_views = r.frame_host()[0].copy()
    assert (from_views[50:290, 1165:1405] != 255).any() and (from_views[290:530, 1165:1405] != 255).any()      # both panels drawn
    r.render(**dict(item, value=st.value.clone(), dd_wt=st.dd_wt.clone()))
    assert np.array_equal(r.frame_host()[0], from_views)
    st.reset()
    assert st.target_pred is None and st.dd_wt is None and st.value is None


def _chain_helper(chain, tmp_path=None, visualize=0):
    from peanut_amd.agent_helper import Agent_Helper
    from peanut_amd.agent_state import Agent_State
    args = SimpleNamespace(**pc.cfg_args(chain["cfg"]))
    args.visualize = visualize
    if visualize:
        args.dump_location, args.exp_name, args.prediction_window = str(tmp_path), "exp", pc.FULL
    state = pw.state_stand_in(args)
    m = pc.local_size(chain["cfg"])
    state.full_w = state.full_h = pc.FULL
    state.local_map = torch.zeros((4 + args.num_sem_categories, m, m), device=DEV)
    state.target_pred = state.value = state.dd_wt = None
    state.vis_item = types.MethodType(Agent_State.vis_item, state)
    h = Agent_Helper(args, state, rank=3, legend=vc.legend())
    h.reset()
    return h, m


def test_plan_act_with_visualize_2_writes_a_frame_per_step_and_plans_the_same(tmp_path):
    from PIL import Image
    chain = pc.chains()["angles"]
    actions = {}
    for visualize in (0, 2):
        h, m = _chain_helper(chain, tmp_path, visualize)
        np.random.seed(chain["cfg"]["seed"])
        actions[visualize] = []
        for k, s in enumerate(chain["steps"]):
            h._get_stg = lambda planner_inputs, step, s=s: (s["stg"], bool(s["stop"]))
            inputs = {'obstacle': torch.zeros((m, m), device=DEV), 'goal': torch.zeros((m, m), dtype=torch.uint8, device=DEV),
                      'pose_pred': np.array(list(s["pose"]) + s["lmb"], np.float64), 'found_goal': s["found"], 'goal_name': 'chair'}
            actions[visualize].append(h.plan_act(inputs)['action'])
            if visualize:
                fn = os.path.join(str(tmp_path), "dump", "exp", "episodes", "thread_3", "eps_0", f"3-0-Vis-{k + 1}.jpg")
                assert os.path.isfile(fn), fn
                with Image.open(fn) as img:
                    assert img.size == (1415, 600) and np.asarray(img).shape == (600, 1415, 3)
                assert h.vis_image.shape == (600, 1415, 3) and h.vis_image.dtype == np.uint8
                # the visited line of this step is in the frame's map panel (index 3 -> palette entry 3, BGR)
                assert (h.vis_image[50:530, 670:1150] == pv.palette_lut()[3][::-1]).all(axis=2).any()
    assert actions[2] == actions[0]
    assert len(os.listdir(os.path.join(str(tmp_path), "dump", "exp", "episodes", "thread_3", "eps_0"))) == len(chain["steps"])


def test_plan_act_batch_renders_its_episodes_in_one_batch(tmp_path):
    from peanut_amd.agent_helper import plan_act_batch
    chains = [pc.chains()[n] for n in ("walk_edges", "thresholds", "window_moves")]
    made = [_chain_helper(c, tmp_path, 1) for c in chains]
    alone = [_chain_helper(c, tmp_path, 1) for c in chains]
    for k in range(2):
        ins = []
        for c, (h, m) in zip(chains, made):
            s = c["steps"][k]
            ins.append({'obstacle': torch.zeros((m, m), device=DEV), 'goal': torch.zeros((m, m), dtype=torch.uint8, device=DEV),
                        'pose_pred': np.array(list(s["pose"]) + s["lmb"], np.float64), 'found_goal': s["found"], 'goal_name': 'chair'})
        script = lambda helpers, inputs, steps, k=k: [(c["steps"][k]["stg"], bool(c["steps"][k]["stop"])) for c in chains]
        outs = plan_act_batch([h for h, _ in made], ins, stg_batch=script)
        for e, (c, (h, m)) in enumerate(zip(chains, alone)):
            s = c["steps"][k]
            h._get_stg = lambda planner_inputs, step, s=s: (s["stg"], bool(s["stop"]))
            assert h.plan_act(ins[e]) == outs[e]
            assert np.array_equal(h.vis_image, made[e][0].vis_image), (k, e)
