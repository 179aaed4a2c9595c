"""Every stream-ordered entry point of include/peanut_hip.h behind a backlogged side stream (tests/stream_cases.py).

Nearly every other GPU test runs on torch's default stream -- the legacy null stream, against which everything orders itself -- or
synchronises before and after each call, so the queue is empty whenever the library enqueues.  A kernel launched on stream 0 instead of
``s``, a dropped hipStreamWaitEvent, a side stream never joined, scratch shared by two calls in flight or a workspace regrown under
in-flight work all give today's bits there.  Here every call is made on a fresh non-blocking stream behind a 50 ms delay:

  P1  late input, early overwrite: the input is produced on the caller's stream BEHIND the delay and overwritten right after the call
      returns; "async" rows must also return while the delay is still pending (they do not secretly synchronise);
  P2  back to back on one fresh handle with no host synchronisation: shape A, a larger shape B, shape A again;
  P3  two handles on two streams, each behind its own delay, enqueued alternately.

The values themselves are held to their oracles by the tests that own these cases; the assertion here is bit equality with the same
call made on an idle default stream, so no tolerance appears anywhere.  The rows are named by their C symbols (tests/test_streams_cpu.py
checks that every "async" and "syncs" row of ``CONTRACT`` is named here):

  convs        peanut_conv_forward
  prediction   peanut_pred_forward, peanut_pred_debug_read
  detector     peanut_rcnn_preprocess, peanut_rcnn_forward_front, peanut_rcnn_inference, peanut_rcnn_semantic, peanut_roi_align,
               peanut_nms, peanut_nms_segments, peanut_paste_masks, peanut_seg_accumulate
  mapping      peanut_preprocess_obs, peanut_preprocess_obs_batch, peanut_map_forward, peanut_map_forward_batch, peanut_map_mark_agent,
               peanut_map_mark_agent_batch
  goal solver  peanut_goal_traversible, peanut_fmm_distance, peanut_goal_select, peanut_goal_select_begin, peanut_goal_select_batch,
               peanut_goal_select_begin_batch
  planner      peanut_goal_map, peanut_goal_map_batch, peanut_stg_traversible, peanut_stg_goal, peanut_stg_window, peanut_stg_plan

Shown to bite with mutants built aside (stale data reaches arithmetic only; each ran once):
  (a) without the hipStreamWaitEvent(h->side, h->ev_fork) of peanut_pred_forward, 14 of the 18 prediction cases the module had then fail (every
      case with the head overlap or graph mode; the overlap_off cases have no side stream).  tests/test_pred_gpu.py sees this fault too, at its
      large shapes only (17 of 60 fail: the handle's side stream is non-blocking, so it is not ordered against the null stream either);
      at 72 x 104 and 96 x 96 only the cases here do.
  (b) without the hipStreamWaitEvent(s, g->ev_field) of peanut_goal_select nothing fails, here or in tests/test_goal_gpu.py and
      tests/test_goal_batch_gpu.py: the solver reads its convergence counters back after every batch of rounds, so the host has
      synchronised the handle's stream before solve_field returns and the weights are enqueued; the wait is redundant as long as the
      solver polls.
  (c) with the split-K reduce of csrc/conv_common.h launched on stream 0, seven conv cases fail (igemm_split_k, pw_two_sources, both
      register-split GEMMs under P1; pw_two_sources, winograd4_overhang, rs_gemm_fp16x3 under P2) while all 220 tests of
      tests/test_conv_gpu.py pass.
  (d) with ev_inputs of peanut_goal_select_begin recorded on stream 0, test_goal_select_begin_then_unrelated_work_then_select[goal_big]
      fails (another goal cell) while the 81 tests of the two goal modules pass; the 64 x 40 case and the agent scenarios pass (the
      handle's stream may share a hardware queue with the backlogged one -- DESIGN.md sec. 10 -- and in the agent a host read-back
      precedes the begin).
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import stream_cases as sc
import test_conv_gpu as tc
import test_mapping_batch_gpu as tmb
import test_workspace_gpu as tw

pytestmark = pytest.mark.gpu


def _inputs(name, seed):
    return sc.to_device(sc.INPUTS[name](seed))


# =====================================================================================================================
# Convs: one case per kernel family, the shapes and option sets of tests/test_workspace_gpu.py
# =====================================================================================================================
def _conv_case(make, B, B2, H, W, c1, cout, c2=0, k=1, stride=1, pad=0, dil=1, residual=False, want=None, prefix=None):
    return dict(make=make, B=B, B2=B2, H=H, W=W, c1=c1, c2=c2, cout=cout, k=k, stride=stride, pad=pad, dil=dil, residual=residual,
                want=want, prefix=prefix)


def _pw_case(case, B2, want, options=None, precision="fp32"):
    B, H, W, cin, cout, stride, relu, residual = case
    return _conv_case(tw._pw(case, options=options, precision=precision), B, B2, H, W, cin, cout, stride=stride, residual=residual, want=want)


def _two_source():
    from peanut_amd.ops import FusedConv
    B, H, W, c1, c2, cout = 1, 23, 17, 256, 512, 1024
    g = torch.Generator().manual_seed(B + H + W + c1 + c2 + cout)
    w = tc._rand((cout, c1 + c2, 1, 1), g, (2.0 / (c1 + c2)) ** 0.5)
    scale, shift = torch.rand(cout, generator=g) + 0.5, tc._rand((cout,), g, 0.1)
    return _conv_case(lambda: FusedConv(w, scale, shift, relu=True), B, 2, H, W, c1, cout, c2=c2, want="conv_pw_glds_128x128")


def _igemm():
    B, H, W, cin, cout, k, s, p, d, relu, residual = tc.CASES[8]
    assert (k, d, cin, cout) == (3, 4, 512, 512)
    return _conv_case(tw._conv3(cin, cout, d, relu, conv_algo="direct"), B, B + 1, H, W, cin, cout, k=3, pad=d, dil=d, residual=residual,
                      prefix="conv_igemm_")


def _wino(tile):
    B, H, W, cin, cout, d, relu, residual = tc.WINO_CASES[1]
    assert (B, H, W, cin, cout) == (1, 15, 13, 256, 320)
    return _conv_case(tw._conv3(cin, cout, d, relu, options={"wino_m": tile}), B, 3, H, W, cin, cout, k=3, pad=d, dil=d, residual=residual)


def _patch():
    B, H, W, cin, cout, s, relu, family = tc.PATCH_CASES[4]
    return _conv_case(tw._conv3(cin, cout, 1, relu, options={"patch_mintiles": 1}, conv_algo="direct", stride=s), B, B + 1, H, W, cin, cout,
                      k=3, stride=s, pad=1, want=family)


CONV_CASES = {
    # split-K with its memset and ordered reduce, dilation 4
    "igemm_split_k": _igemm,
    # the two-source form, ragged M, split-K
    "pw_two_sources": _two_source,
    # the stream-K tail: 416 tiles, 160 tail tiles in runs of 10
    "pw256p_stream_k_tail": lambda: _pw_case((13, 64, 64, 512, 256, 1, True, False), 14, "conv_pw_glds_256x128p", options=tc.P256P_OPTS),
    # nothing but raw partial tiles and the reduce
    "pw256wp_partials": lambda: _pw_case(tc.WP_CASES[5], 3, "conv_pw_glds_256x256p", options=tc.WP_OPTS),
    # a residual on the A-resident kernel
    "pw_ares_residual": lambda: _pw_case(tc.ARES_CASES[2], 9, "conv_pw_ares_128x128"),
    "patch_ragged": _patch,
    # Winograd with tiles that overhang the map; batch 3 regrows V and M
    "winograd4_overhang": lambda: _wino(4),
    "winograd6_overhang": lambda: _wino(6),
    # one register-split GEMM per emulated precision: split-K over 128 k-tiles; the 256 x 256 split-K tail
    "rs_gemm_bf16x6": lambda: _pw_case(tw._RS_GEMMS[1][0], tw._RS_GEMMS[1][0][0] + 1, "gemm_rs6_128x128", precision="bf16x6"),
    "rs_gemm_fp16x3": lambda: _pw_case(tw._RS_GEMMS[2][0], tw._RS_GEMMS[2][0][0] + 1, "gemm_rs3h_256x256", precision="fp16x3"),
}


def conv_shapes(c, b):
    """The shapes of (x[, x2][, residual]) of a conv case at batch ``b``."""
    def o(n):
        return (n + 2 * c["pad"] - c["dil"] * (c["k"] - 1) - 1) // c["stride"] + 1
    shapes = [(b, c["H"], c["W"], c["c1"])]
    if c["c2"]:
        shapes.append((b, c["H"], c["W"], c["c2"]))
    if c["residual"]:
        shapes.append((b, o(c["H"]), o(c["W"]), c["cout"]))
    return shapes


def _conv_run(c):
    def run(conv, x, outs):
        rest = list(x[1:])
        x2 = rest.pop(0) if c["c2"] else None
        res = rest.pop(0) if c["residual"] else None
        y = conv(x[0], x2=x2, residual=res)
        if x[0].shape[0] == c["B"]:          # the family this case is about (thread-local host state: no synchronisation)
            fam = tc._last_kernel()
            assert c["want"] is None or fam == c["want"], fam
            assert c["prefix"] is None or fam.startswith(c["prefix"]), fam
        return y
    return run


@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv_late_input_early_overwrite(name):
    """P1 on peanut_conv_forward, one case per kernel family."""
    c = CONV_CASES[name]()
    build = sc.randn(conv_shapes(c, c["B"]))
    sc.p1(f"conv {name}", c["make"], _conv_run(c), sc.to_device(build(0)), sc.to_device(build(1)), sc.klass("peanut_conv_forward"))


@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv_back_to_back(name):
    """P2 on peanut_conv_forward: batch B, a larger batch (another split plan, regrown Winograd scratch), batch B again."""
    c = CONV_CASES[name]()
    xs = [sc.to_device(sc.randn(conv_shapes(c, b))(seed)) for seed, b in enumerate((c["B"], c["B2"], c["B"]))]
    assert c["B2"] > c["B"]
    sc.p2(f"conv {name}", c["make"], _conv_run(c), xs)


def test_conv_two_handles_two_streams():
    """P3: a split-K pointwise handle and a Winograd handle, each on its own stream."""
    cases = [CONV_CASES["pw_two_sources"](), CONV_CASES["winograd4_overhang"]()]
    xs = [sc.to_device(sc.randn(conv_shapes(c, c["B"]))(i)) for i, c in enumerate(cases)]
    sc.p3("conv", [c["make"] for c in cases], [_conv_run(c) for c in cases], xs)


# =====================================================================================================================
# Prediction forward
# =====================================================================================================================
PRED_MODES = ["overlap_on", "overlap_off", "graph"]


_pred_models = {}


def _pred_make(precision, mode, keep=False, fresh=False):
    """A factory of prediction models in ``mode``.  Unless ``fresh``, the module keeps ONE model per precision and sets it up anew for
    every case (head overlap, graph mode, debug taps; changing an option drops the handle's cached plans): creating a model costs
    more than all the forwards of a case.  P2 asks for fresh handles: they must meet every shape for the first time in flight."""
    def make():
        if fresh or precision not in _pred_models:
            m = tw._pred_model(**({} if precision == "fp32" else dict(precision=precision)))
            if not fresh:
                _pred_models[precision] = m
        else:
            m = _pred_models[precision]
        m.model.use_graph(False)
        m.model.debug_keep(keep)
        m.model.set_option("ppm_overlap", 0 if mode == "overlap_off" else 1)          # the option behind PEANUT_PPM_OVERLAP
        m.model.use_graph(mode == "graph")
        m._outs = {}
        return m
    return make


def _pred_run(m, x, outs):
    """peanut_pred_forward into a buffer that stays the same for the same input buffer (graph mode caches per (in, out) pair)."""
    key = x[0].data_ptr()
    if key not in m._outs:
        m._outs[key] = torch.empty((x[0].shape[0], 6) + tuple(x[0].shape[2:]), device="cuda")
    return m.get_prediction_batch(x[0], apply_sigmoid=False, out=m._outs[key])


@pytest.mark.parametrize("precision", ["fp32", "fp16x3"])
@pytest.mark.parametrize("inp", ["pred_rect", "pred_96"])
@pytest.mark.parametrize("mode", PRED_MODES)
def test_prediction_late_input_early_overwrite(mode, inp, precision):
    """P1 on peanut_pred_forward: rect_72x104 (B = 2) and 1 x 96 x 96 (batch 1: the pyramid GEMMs run on gemm_skinny on the head's side
    stream), with the head overlap on and off, and in graph mode three times -- direct, captured, replayed -- each behind its own
    backlog.  fp16x3 carries the range flag; its logits here are finite, as r_good's are."""
    good, stale = _inputs(inp, 0), _inputs(inp, 1)

    def after(m):
        assert bool(torch.isfinite(m._outs[next(iter(m._outs))]).all())
        if (mode, inp, precision) == ("overlap_on", "pred_96", "fp32"):
            fam = {n: k for n, k, *_ in m.model.profile(good[0])}
            pyramid = [k for n, k in fam.items() if "psp_modules" in n or "bottleneck.conv[ppm" in n]
            assert pyramid and all(k == "gemm_skinny" for k in pyramid), pyramid
    graph = mode == "graph"
    sc.p1(f"pred {mode} {inp} {precision}", _pred_make(precision, mode), _pred_run, good, stale, sc.klass("peanut_pred_forward"),
          reps=3 if graph else 1, warm=not graph, after=after)


@pytest.mark.parametrize("precision", ["fp32", "fp16x3"])
@pytest.mark.parametrize("mode", PRED_MODES)
def test_prediction_back_to_back_across_an_arena_regrowth(mode, precision):
    """P2: rect_72x104 three times (graph mode: direct, captured, replayed), then test_workspace_gpu.BIG_MAP, which regrows the arena
    and must drop the cached graphs while the earlier forwards are still queued, then another rect_72x104 input three times."""
    assert tw.BIG_MAP == (1, 200, 200)
    a, big, a3 = _inputs("pred_rect", 0), _inputs("pred_big", 1), _inputs("pred_rect", 2)
    sc.p2(f"pred {mode} {precision}", _pred_make(precision, mode, fresh=True), _pred_run, [a, a, a, big, a3, a3, a3],
          plain_make=_pred_make(precision, mode))


def test_prediction_debug_read_late_input():
    """P1 on peanut_pred_debug_read (with the forward that fills the tap)."""
    def run(m, x, outs):
        y = _pred_run(m, x, outs)
        return [y, m.model.debug_tensor("layer1")]
    assert sc.klass("peanut_pred_debug_read") == "async"
    sc.p1("pred debug_read", _pred_make("fp32", "overlap_on", keep=True), run, _inputs("pred_96", 0), _inputs("pred_96", 1), "async")


def test_prediction_two_handles_two_streams():
    """P3: two models (fp32 with the head overlap; fp16x3 in graph mode), each on its own stream behind its own backlog."""
    sc.p3("pred", [_pred_make("fp32", "overlap_on"), _pred_make("fp16x3", "graph")], [_pred_run, _pred_run],
          [_inputs("pred_rect", 0), _inputs("pred_96", 1)], rounds=3)


# =====================================================================================================================
# Detector (the small configuration) and its operators
# =====================================================================================================================
_det = {}


def _det_make(fresh=True):
    """The small detector with the front end's side-stream option on."""
    from peanut_amd import _lib
    if "case" not in _det:
        cfg, sd, _ = tw._det_case("small")
        _det["case"] = (cfg, sd)
    cfg, sd = _det["case"]
    if not fresh and "net" in _det:
        return _det["net"]
    with _lib.default_options(rcnn_fpn_overlap=1):
        net = tw._det_net(cfg, sd, "default", "fp32")
    if not fresh:
        _det["net"] = net
    return net


def _run_inference(net, x, outs):
    return net.inference(x[0])


def _run_semantic(net, x, outs):
    sem = net.semantic(x[0], net.cfg.num_classes, 0.0, 0.0, None)
    return [sem, list(net.last_detection_counts)]


DET_ROWS = {
    "peanut_rcnn_preprocess": lambda net, x, outs: net.preprocess(x[0]),
    "peanut_rcnn_forward_front": lambda net, x, outs: [list(t) for t in net.forward_front(x[0])],
    "peanut_rcnn_inference": _run_inference,
    "peanut_rcnn_semantic": _run_semantic,
}


@pytest.mark.parametrize("symbol", list(DET_ROWS))
def test_detector_late_input_early_overwrite(symbol):
    """P1 on the detector's entry points, two 96 x 128 frames: peanut_rcnn_preprocess and peanut_rcnn_forward_front as async rows,
    peanut_rcnn_inference and peanut_rcnn_semantic (they read the detection counts) without the pending assertion."""
    assert sc.klass(symbol) == ("syncs" if symbol in ("peanut_rcnn_inference", "peanut_rcnn_semantic") else "async")
    sc.p1(symbol, lambda: _det_make(fresh=False), DET_ROWS[symbol], _inputs("det_frames", 0), _inputs("det_frames", 1), sc.klass(symbol))


@pytest.mark.parametrize("symbol", ["peanut_rcnn_inference", "peanut_rcnn_semantic"])
def test_detector_back_to_back_across_a_batch_change(symbol):
    """P2 with B = 1, 2, 1: each change of B triggers the synchronous lvl_count upload between queued work."""
    xs = [_inputs("det_frame1", 0), _inputs("det_frames", 1), _inputs("det_frame1", 2)]
    sc.p2(symbol, _det_make, DET_ROWS[symbol], xs)


def test_roi_align_late_input():
    """P1 on peanut_roi_align: four NHWC levels, 50 rois over all of them, 7 x 7 bins."""
    from peanut_amd.rcnn import roi_align_pyramid
    from rcnn_glue import assign_levels
    good, stale = _inputs("roi", 0), _inputs("roi", 1)
    levels = assign_levels(good[4][:, 1:]).to(torch.int32)
    assert set(levels.tolist()) == {0, 1, 2, 3}
    sc.p1("peanut_roi_align", lambda: None, lambda h, x, outs: roi_align_pyramid(list(x[:4]), x[4], levels, 7), good, stale,
          sc.klass("peanut_roi_align"))


def test_nms_late_input():
    """P1 on peanut_nms (one list of 300 boxes) and peanut_nms_segments (four lists, one of them empty)."""
    from peanut_amd import _lib
    from peanut_amd.rcnn import nms_keep_segments
    lib = _lib.load()
    n = 300
    ws = torch.empty((max(int(lib.peanut_nms_workspace_bytes(n)), 8),), dtype=torch.uint8, device="cuda")
    keep = torch.empty((n,), dtype=torch.uint8, device="cuda")

    def single(h, x, outs):
        _lib.check(lib.peanut_nms(x[0].data_ptr(), x[1].data_ptr(), n, 0.5, ws.data_ptr(), keep.data_ptr(), _lib.current_stream_ptr()),
                   "peanut_nms")
        return keep
    sc.p1("peanut_nms", lambda: None, single, _inputs("nms_one", 0), _inputs("nms_one", 1), sc.klass("peanut_nms"), outs=[keep])
    counts = [130, 0, 70, 257]
    sc.p1("peanut_nms_segments", lambda: None, lambda h, x, outs: nms_keep_segments(x[0], x[1], counts, 0.5), _inputs("nms", 0),
          _inputs("nms", 1), sc.klass("peanut_nms_segments"))


def test_paste_masks_and_seg_accumulate_late_input():
    """P1 on peanut_paste_masks and peanut_seg_accumulate."""
    from peanut_amd.rcnn import paste_masks
    from peanut_amd.segmentation import accumulate_instances
    sc.p1("peanut_paste_masks", lambda: None, lambda h, x, outs: paste_masks(x[0], x[1], (60, 84), 0.5), _inputs("paste", 0),
          _inputs("paste", 1), sc.klass("peanut_paste_masks"))
    sc.p1("peanut_seg_accumulate", lambda: None, lambda h, x, outs: accumulate_instances(x[0], x[1], x[2], 9, 0.6, 0.8, 3),
          _inputs("seg", 0), _inputs("seg", 1), sc.klass("peanut_seg_accumulate"))


# =====================================================================================================================
# Mapping
# =====================================================================================================================
_OBS_ARGS = SimpleNamespace(env_frame_width=640, frame_width=160, min_depth=0.5, max_depth=5.0)


def test_preprocess_obs_late_input():
    """P1 on peanut_preprocess_obs and peanut_preprocess_obs_batch (E = 3)."""
    from peanut_amd.agent_helper import preprocess_obs, preprocess_obs_batch
    sc.p1("peanut_preprocess_obs", lambda: None, lambda h, x, outs: preprocess_obs(x[0], x[1], x[2], _OBS_ARGS), _inputs("obs_single", 0),
          _inputs("obs_single", 1), sc.klass("peanut_preprocess_obs"))
    sc.p1("peanut_preprocess_obs_batch", lambda: None, lambda h, x, outs: preprocess_obs_batch(x[0], x[1], x[2], _OBS_ARGS),
          _inputs("obs_batch3", 0), _inputs("obs_batch3", 1), sc.klass("peanut_preprocess_obs_batch"))


def _pose0(E=None):
    p = [12.0, 12.0, 0.0]
    return torch.tensor(p if E is None else [p] * E, device="cuda")


@pytest.mark.parametrize("graph", [False, True], ids=["plain", "graph"])
def test_map_forward_late_input_early_overwrite(graph):
    """P1 on peanut_map_forward: obs, pose_obs and maps_last are produced late and overwritten after the call; the pose is updated in
    place.  With use_graph the same buffers run three times: direct, captured, replayed."""
    pose0 = _pose0()
    pose = pose0.clone()
    outs = [torch.empty((1, 100, 100), device="cuda"), torch.empty((14, 480, 480), device="cuda")]

    def make():
        sm = tmb._module(tmb._args())
        sm.use_graph(graph)
        return sm

    def run(sm, x, outs):
        pose.copy_(pose0)
        fp, mp, _, _ = sm(x[0], x[1][0], x[2][0], pose, None, out=(outs[0], outs[1]))
        return [fp, mp, pose.clone()]
    sc.p1(f"peanut_map_forward graph={graph}", make, run, _inputs("map_single", 0), _inputs("map_single", 1),
          sc.klass("peanut_map_forward"), outs=outs, reps=3 if graph else 1, warm=not graph)


def test_map_forward_batch_late_input_early_overwrite():
    """P1 on peanut_map_forward_batch at E = 4."""
    pose0 = _pose0(4)

    def run(sm, x, outs):
        poses = pose0.clone()
        fp, maps, _, _ = sm.forward_batch(x[0], x[1], [x[2][e] for e in range(4)], poses)
        return [fp, list(maps), poses]
    sc.p1("peanut_map_forward_batch", lambda: tmb._module(tmb._args(), reserve=4), run, _inputs("map_batch4", 0), _inputs("map_batch4", 1),
          sc.klass("peanut_map_forward_batch"))


def _episode(sm, obs, rel, sync):
    """Consecutive frames from an empty map as the agent runs them: two map buffers in turn, the pose in place, one fp buffer."""
    bufs = [torch.zeros(14, 480, 480, device="cuda"), torch.empty(14, 480, 480, device="cuda")]
    fpb, pose, rec = torch.empty((1, 100, 100), device="cuda"), _pose0(), []
    for i in range(obs.shape[0]):
        fp, mp, _, _ = sm(obs[i:i + 1], rel[i], bufs[i % 2], pose, None, out=(fpb, bufs[(i + 1) % 2]))
        rec.append([fp.clone(), mp.clone(), pose.clone()])
        if sync:
            torch.cuda.synchronize()
    return rec, bufs


@pytest.mark.parametrize("graph", [False, True], ids=["plain", "graph"])
def test_map_forward_consecutive_frames_without_a_host_sync(graph, golden_dir):
    """P2 on peanut_map_forward: the first golden frames of seq0 (three; six in graph mode, so that each of the two cached graphs is
    captured and replayed) through two ping-ponged map buffers behind one backlog, no host synchronisation at all."""
    obs, rel, _ = tw._golden_frames(golden_dir, "seq0", 6 if graph else 3)
    plain, _ = _episode(tmb._module(tmb._args()), obs, rel, sync=True)
    assert float(plain[-1][1][4:].sum()) > 0 and not sc.same(plain[0], plain[-1])
    sm = tmb._module(tmb._args())
    sm.use_graph(graph)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        sc.backlog(side)
        got, keep = _episode(sm, obs, rel, sync=False)
        side.synchronize()
    sc.assert_same(got, plain, f"consecutive frames, graph={graph}")
    torch.cuda.synchronize()


def test_map_projection_two_handles_two_streams():
    """P3: two Semantic_Mapping handles, each on its own stream."""
    pose0 = _pose0()

    def run(sm, x, outs):
        pose = pose0.clone()
        fp, mp, _, _ = sm(x[0], x[1][0], x[2][0], pose, None)
        return [fp, mp, pose]
    make = lambda: tmb._module(tmb._args())  # noqa: E731
    sc.p3("map projection", [make, make], [run, run], [_inputs("map_single", 0), _inputs("map_single", 1)])


def _mark_setup():
    from peanut_amd.agent_state import disk
    rad = 5                                            # col_rad + 1 of the agent's default
    return rad, torch.from_numpy(np.ascontiguousarray(disk(rad))).cuda()


def test_mark_agent_late_input(golden_dir):
    """P1 on peanut_map_mark_agent and peanut_map_mark_agent_batch (E = 3) on three golden frames: the local maps are what the
    projection leaves after frames 1, 2 and 3 of seq0 (good) and of seq1 (stale); they are written in place."""
    from peanut_amd import _lib
    lib = _lib.load()
    sm = tmb._module(tmb._args())
    good3 = [r[1] for r in tw._map_run(sm, *tw._golden_frames(golden_dir, "seq0")[:2])]
    stale3 = [r[1] for r in tw._map_run(sm, *tw._golden_frames(golden_dir, "seq1")[:2])]
    assert len(good3) == 3 and float(good3[-1][4:].sum()) > 0
    rad, selem = _mark_setup()
    m = 480
    centres = (C.c_int * 4)(240, 240, 300, 20)

    def single(h, x, outs):
        rc = lib.peanut_map_mark_agent(x[0].data_ptr(), 14, m, 238, 243, 238, 243, selem.data_ptr(), rad, 2, C.byref(centres),
                                       _lib.current_stream_ptr())
        _lib.check(rc, "peanut_map_mark_agent")
        return x[0].clone()
    sc.p1("peanut_map_mark_agent", lambda: None, single, good3[2:], stale3[2:], sc.klass("peanut_map_mark_agent"))
    squares = (C.c_int * 12)(238, 243, 238, 243, 0, 3, 475, 480, 98, 103, 375, 380)
    n_c = (C.c_int * 3)(1, 0, 2)
    cs = (C.c_int * 12)(240, 240, 0, 0, 0, 0, 0, 0, 100, 377, 300, 20)

    def batch(h, x, outs):
        ptrs = (C.c_void_p * 3)(*[t.data_ptr() for t in x])
        rc = lib.peanut_map_mark_agent_batch(3, ptrs, 14, m, squares, selem.data_ptr(), rad, n_c, cs, _lib.current_stream_ptr())
        _lib.check(rc, "peanut_map_mark_agent_batch")
        return [t.clone() for t in x]
    sc.p1("peanut_map_mark_agent_batch", lambda: None, batch, good3, stale3, sc.klass("peanut_map_mark_agent_batch"))


# =====================================================================================================================
# Goal solver, at the shapes of the goal cases of tests/test_workspace_gpu.py
# =====================================================================================================================
GOAL_SHAPES = {"goal_small": sc.GOAL_SMALL, "goal_big": sc.GOAL_BIG}


def _solver(key):
    from peanut_amd.goal import GeodesicSolver
    h, w = GOAL_SHAPES[key]["shape"]
    return lambda: GeodesicSolver(h, w, 2)


def _no_rounds(res):
    """A select's result without ``rounds``: the number of relaxation rounds a solve enqueues follows the round hints the handle kept
    from its last solve (include/peanut_hip.h: "its round hints"), so it depends on the handle's history by design; the field, the
    value map, the goal, the weights' sum, the keep-last flag, the pass count and the convergence flag do not."""
    return {k: v for k, v in res.items() if k != "rounds"}


def _select(key, want=True):
    g = GOAL_SHAPES[key]
    return lambda sol, x, outs: _no_rounds(sol.select(x[0], x[1], None, g["lmb"], g["loc"], x[2], 500.0, 5, want_dist=want, want_value=want))


@pytest.mark.parametrize("key", list(GOAL_SHAPES))
def test_goal_solver_late_input_early_overwrite(key):
    """P1 on peanut_goal_traversible (async), peanut_fmm_distance and peanut_goal_select (both synchronise the caller's stream)."""
    g = GOAL_SHAPES[key]
    good, stale = _inputs(key, 0), _inputs(key, 1)
    sc.p1(f"peanut_goal_traversible {key}", _solver(key), lambda sol, x, outs: sol.traversible(x[0], x[1], None), good, stale,
          sc.klass("peanut_goal_traversible"))
    assert sc.klass("peanut_fmm_distance") == sc.klass("peanut_goal_select") == "syncs"

    def distance(sol, x, outs):
        trav = sol.traversible(x[0], x[1], None)
        return [trav, sol.distance(trav, goal=g["loc"], fill_max_plus_one=True)]
    sc.p1(f"peanut_fmm_distance {key}", _solver(key), distance, good, stale, "syncs")
    sc.p1(f"peanut_goal_select {key}", _solver(key), _select(key), good, stale, "syncs")


def _late(side, x, good):
    """A backlog on ``side`` and, behind it, the inputs produced on that stream."""
    ev = sc.backlog(side)
    for xi, g in zip(x, good):
        xi.copy_(g, non_blocking=True)
    return ev


@pytest.mark.parametrize("key", list(GOAL_SHAPES))
def test_goal_select_begin_then_unrelated_work_then_select(key):
    """peanut_goal_select_begin -> unrelated queued work (a second backlog) -> peanut_goal_select: the map inputs are produced late
    on the caller's stream and overwritten right after the select; the begin returns while the backlog is pending; the field begun
    on the handle's own stream is taken over (begun_matches) and joined before the weights."""
    g = GOAL_SHAPES[key]
    good, stale = _inputs(key, 0), _inputs(key, 1)
    sol = _solver(key)()
    run = _select(key)
    r_good = sc.snapshot(run(sol, good, None))
    r_stale = sc.snapshot(run(sol, stale, None))
    torch.cuda.synchronize()
    assert not sc.same(r_good, r_stale)
    x = [t.clone() for t in stale]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert sc.klass("peanut_goal_select_begin") == "async"
    with torch.cuda.stream(side):
        for rep in range(2):                          # (the second one is the steady-state call)
            before = sol.begun_matches
            ev = _late(side, x[:2], good[:2])
            sol.select_begin(x[0], x[1], None, g["lmb"], g["loc"])
            pending = not ev.query()
            sc.backlog(side)
            x[2].copy_(good[2], non_blocking=True)     # target_pred arrives after the unrelated work
            res = run(sol, x, None)
            for xi, s in zip(x, stale):
                xi.copy_(s, non_blocking=True)
            side.synchronize()
            assert sol.begun_matches == before + 1
            sc.assert_same(res, r_good, f"begin / select {key}, call {rep}")
    assert pending, "peanut_goal_select_begin returned only after the backlog had drained: it synchronises"
    torch.cuda.synchronize()


def test_goal_select_begin_for_one_input_then_select_for_another():
    """The begun work is for other buffers: the select lets it run out and solves its own inputs."""
    key = "goal_small"
    g = GOAL_SHAPES[key]
    a, b = _inputs(key, 0), _inputs(key, 1)
    sol = _solver(key)()
    run = _select(key)
    want = sc.snapshot(run(sol, b, None))
    torch.cuda.synchronize()
    xa, xb = [t.clone() for t in b], [t.clone() for t in a]          # (both hold the other's data until the late copies)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        before = sol.begun_matches
        _late(side, xa + xb, a + b)
        sol.select_begin(xa[0], xa[1], None, g["lmb"], g["loc"])
        res = run(sol, xb, None)
        for xi, s in zip(xa + xb, b + a):
            xi.copy_(s, non_blocking=True)
        side.synchronize()
    assert sol.begun_matches == before
    sc.assert_same(res, want, "select after a begin for other inputs")
    torch.cuda.synchronize()


def test_goal_select_batch_begun_behind_a_backlog():
    """peanut_goal_select_begin_batch / peanut_goal_select_batch at E = 3, the map inputs late and overwritten after the select."""
    from peanut_amd.goal import select_batch, select_begin_batch
    g = sc.GOAL_BIG
    good, stale = _inputs("goal_big3", 0), _inputs("goal_big3", 1)
    sols = [_solver("goal_big")() for _ in range(3)]

    def items(x):
        return [(x[3 * e], x[3 * e + 1], None, g["lmb"], (g["loc"][0] + 10 * e, g["loc"][1] - 20 * e)) for e in range(3)]

    def run(x):
        return [_no_rounds(r) for r in select_batch(sols, items(x), [x[3 * e + 2] for e in range(3)], 500.0, 5, want_dist=True, want_value=True)]
    r_good, r_stale = sc.snapshot(run(good)), sc.snapshot(run(stale))
    torch.cuda.synchronize()
    assert not sc.same(r_good, r_stale)
    x = [t.clone() for t in stale]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert sc.klass("peanut_goal_select_begin_batch") == "async" and sc.klass("peanut_goal_select_batch") == "syncs"
    with torch.cuda.stream(side):
        for rep in range(2):
            before = [s.begun_matches for s in sols]
            ev = _late(side, x, good)
            select_begin_batch(sols, items(x))
            pending = not ev.query()
            sc.backlog(side)
            res = run(x)
            for xi, s in zip(x, stale):
                xi.copy_(s, non_blocking=True)
            side.synchronize()
            assert [s.begun_matches for s in sols] == [b + 1 for b in before]
            sc.assert_same(res, r_good, f"begin_batch / select_batch, call {rep}")
    assert pending, "peanut_goal_select_begin_batch returned only after the backlog had drained: it synchronises"
    torch.cuda.synchronize()


def test_goal_solver_back_to_back_and_two_handles():
    """P2: three selects in a row on one handle with no host synchronisation between the calls but the library's own; P3: two solvers
    of different map sizes, each on its own stream."""
    sc.p2("goal select", _solver("goal_small"), _select("goal_small"), [_inputs("goal_small", s) for s in range(3)])
    sc.p3("goal select", [_solver("goal_small"), _solver("goal_big")], [_select("goal_small"), _select("goal_big")],
          [_inputs("goal_small", 0), _inputs("goal_big", 1)])


# =====================================================================================================================
# The planner inputs: goal map on strided views, short-term goal
# =====================================================================================================================
def _gm_view(parent):
    m = parent.shape[1] // 2
    return parent[:, 7:7 + m, m - 3:2 * m - 3]


def test_goal_map_on_strided_views_late_input():
    """P1 on peanut_goal_map and peanut_goal_map_batch (E = 3): the local maps are views into larger tensors, read in place."""
    import goal_map_cases as gmc
    from peanut_amd import _lib
    lib = _lib.load()
    cases = gmc.random_cases()
    m = gmc.M_RANDOM

    def params(k):
        c = cases[k]
        return [c["cn"], c["morph"], c["n_erode"], c["detect"], c["goal"][0], c["goal"][1]]
    outs = [torch.empty((m, m), dtype=torch.uint8, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")]

    def single(h, x, outs):
        v = _gm_view(x[0])
        assert not v.is_contiguous()
        rc = lib.peanut_goal_map(v.data_ptr(), gmc.C, m, int(v.stride(0)), int(v.stride(1)), *params(0), outs[0].data_ptr(),
                                 outs[1].data_ptr(), _lib.current_stream_ptr())
        _lib.check(rc, "peanut_goal_map")
        return outs
    sc.p1("peanut_goal_map", lambda: None, single, _inputs("goal_map_view", 0), _inputs("goal_map_view", 1), sc.klass("peanut_goal_map"),
          outs=outs)
    E = 3
    outs = [torch.empty((m, m), dtype=torch.uint8, device="cuda") for _ in range(E)] + [torch.empty(E, dtype=torch.int32, device="cuda")]
    pr = (C.c_int * (6 * E))(*[v for e in range(E) for v in params(2 * e)])
    op = (C.c_void_p * E)(*[t.data_ptr() for t in outs[:E]])

    def batch(h, x, outs):
        views = [_gm_view(p) for p in x]
        ptrs = (C.c_void_p * E)(*[v.data_ptr() for v in views])
        ps = (C.c_longlong * E)(*[int(v.stride(0)) for v in views])
        rs = (C.c_longlong * E)(*[int(v.stride(1)) for v in views])
        rc = lib.peanut_goal_map_batch(E, ptrs, gmc.C, m, ps, rs, pr, op, outs[E].data_ptr(), _lib.current_stream_ptr())
        _lib.check(rc, "peanut_goal_map_batch")
        return outs
    sc.p1("peanut_goal_map_batch", lambda: None, batch, _inputs("goal_map_views3", 0), _inputs("goal_map_views3", 1),
          sc.klass("peanut_goal_map_batch"), outs=outs)


def test_short_term_goal_operators_late_input():
    """P1 on peanut_stg_traversible, peanut_stg_goal and peanut_stg_window as async rows."""
    import stg_cases
    from peanut_amd import _lib
    from peanut_amd.planner import stg_goal, stg_traversible
    lib = _lib.load()
    c = stg_cases.mask_cases()[0]
    good, stale = _inputs("stg_masks", 0), _inputs("stg_masks", 1)
    sc.p1("peanut_stg_traversible", lambda: None,
          lambda h, x, outs: stg_traversible(x[0], (c["full"], c["full"]), c["lmb"], c["col_rad"], x[2], x[3], c["start_exact"]),
          good, stale, sc.klass("peanut_stg_traversible"))
    sc.p1("peanut_stg_goal", lambda: None, lambda h, x, outs: stg_goal(x[1], 2), good, stale, sc.klass("peanut_stg_goal"))
    res = torch.empty(C.sizeof(_lib.StgWindowC), dtype=torch.uint8, device="cuda")

    def window(h, x, outs):
        rc = lib.peanut_stg_window(x[0].data_ptr(), int(x[0].shape[0]), 30.5, 30.25, stg_cases.STEP_SIZE, outs[0].data_ptr(),
                                   _lib.current_stream_ptr())
        _lib.check(rc, "peanut_stg_window")
        return outs[0]
    sc.p1("peanut_stg_window", lambda: None, window, _inputs("stg_fields", 0), _inputs("stg_fields", 1), sc.klass("peanut_stg_window"),
          outs=[res])


def test_short_term_goal_plan_on_the_retry_scene():
    """P1 (without the pending assertion) and P2 on peanut_stg_plan: the blocked_start scene of tests/stg_cases.py, which takes two
    solves and a host decision between them in one call."""
    import stg_cases
    from peanut_amd.planner import ShortTermGoal
    c = next(s for s in stg_cases.scene_cases() if s["name"] == "blocked_start")
    assert c["expect_retry"] == 1 and sc.klass("peanut_stg_plan") == "syncs"
    args = SimpleNamespace(map_size_cm=c["full"] * 5, map_resolution=5, global_downscaling=2, col_rad=c["col_rad"],
                           magnify_goal_when_hard=stg_cases.MAGNIFY_WHEN_HARD)

    def run(p, x, outs):
        p.get_stg(x[0], x[1], x[2], x[3], c["lmb"], c["start_exact"], c["found_goal"], c["goal_name"], taps=True)
        return dict(p.last)
    good = _inputs("stg_scenes", 0)
    make = lambda: ShortTermGoal(args, device="cuda:0")  # noqa: E731
    p = sc.p1("peanut_stg_plan", make, run, good, _inputs("stg_scenes", 1), "syncs")
    assert run(p, good, None)["retried"] == 1 and p.last["n_solves"] >= 2
    sc.p2("peanut_stg_plan", make, run, [good, _inputs("stg_scenes", 1), _inputs("stg_scenes", 2)])


# =====================================================================================================================
# The Python layer: whole agent steps behind a backlog
# =====================================================================================================================
_agent_model = []


def _agent_setup(plan):
    from oracle.agent_ref import agent_args
    from peanut_amd.prediction import PEANUT_Prediction_Model
    from peanut_amd.weights import PredCfg, make_seeded_state_dict
    args = agent_args(only_explore=0, prediction_window=240, map_size_cm=2400, select_goal=True, num_local_steps=5, goal_map=True,
                      goal_erode=3, plan_stg=plan)
    if not _agent_model:
        _agent_model.append(PEANUT_Prediction_Model(args, state_dict=make_seeded_state_dict(PredCfg(), 0)))
    return args, _agent_model[0]


def _record(s, goal, predicted, plan):
    """What a step leaves behind: maps, poses, goals, the found flag and, with ``plan``, the planner's short-term goal and stop flag.
    They stand for the action: the state machine that turns them into one (Agent_Helper._plan) is the caller's, not this package's.
    Short-term planning synchronises (peanut_stg_plan), as it does in an agent that plans; without ``plan`` nothing here touches the
    host -- device clones only -- so the step that follows meets exactly the synchronisations update_state itself makes."""
    from peanut_amd.peanut_agent import coco_goal_names
    rec = dict(local_map=s.local_map.clone(), full_map=s.full_map.clone(), local_pose=s.local_pose.clone(), full_pose=s.full_pose.clone(),
               lmb=[int(v) for v in s.lmb], goals=[list(map(int, g)) for g in s.global_goals], found=int(s.found_goal),
               goal_map=s.goal_map.clone(), target_pred=None if s.target_pred is None else s.target_pred.clone(),
               predicted=bool(predicted), cell=(s.loc_r, s.loc_c))
    if plan:
        stg, stop = s.short_term_goal({"goal_name": coco_goal_names.get(int(goal), "")})
        rec.update(stg=tuple(float(v) for v in stg), stop=bool(stop))
    return rec


def _in_a_backlogged_stream(scenario):
    """``scenario(before_step)`` once plainly and once inside a side stream with a backlog enqueued before every step."""
    plain = scenario(lambda: None)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = scenario(lambda: sc.backlog(side))
        side.synchronize()
    torch.cuda.synchronize()
    return plain, got


@pytest.mark.parametrize("plan", [True, False], ids=["plan_stg", "no_host_work_between_steps"])
def test_single_episode_behind_a_backlog_before_every_step(plan):
    """The scenario of test_replay_loop_runs_full_pipeline (tests/test_agent_gpu.py) with select_goal, goal_map and (plan) plan_stg on: after
    every step maps, poses, goals, found flag and short-term goal equal the plain run's.  Holds Agent_State._upload_pose (one pinned
    buffer under non_blocking=True), _found_host, ShortTermGoal and the wrappers' temporaries to what their comments claim."""
    import test_lockstep_gpu as tl
    from peanut_amd.agent_state import Agent_State
    from peanut_amd.replay import run_episode
    args, model = _agent_setup(plan)
    frames = tl._episodes()[0]

    def scenario(before_step):
        st, steps = Agent_State(args, prediction_model=model), []

        def on_step(i, s, predicted):
            steps.append(_record(s, 1, predicted, plan))
            before_step()
        before_step()
        n = run_episode(st, frames, goal_cat=1, on_step=on_step)
        return [n, steps]
    plain, got = _in_a_backlogged_stream(scenario)
    assert plain[0] >= 2 and len(plain[1]) == len(frames) and float(plain[1][-1]["local_map"][4:].sum()) > 0
    for i, (a, b) in enumerate(zip(got[1], plain[1])):
        sc.assert_same(a, b, f"step {i}")
    assert got[0] == plain[0]


@pytest.mark.parametrize("plan", [True, False], ids=["plan_stg", "no_host_work_between_steps"])
def test_lockstep_episodes_behind_a_backlog_before_every_step(plan):
    """The lock-step scenario of tests/test_lockstep_gpu.py at E = 2 (12 and 9 frames) with goal_map and plan_stg on, the same way:
    holds Agent_State_Group._upload_poses and its batched goal selection and goal maps."""
    import test_lockstep_gpu as tl
    from peanut_amd.agent_state import Agent_State
    from peanut_amd.replay import run_episodes
    args, model = _agent_setup(plan)
    eps, goals = tl._episodes()[:2], tl.GOALS[:2]

    def scenario(before_step):
        states, steps = [Agent_State(args, prediction_model=model) for _ in range(2)], []

        def on_step(i, act, predicted):
            steps.append([_record(s, goals[states.index(s)], p, plan) for s, p in zip(act, predicted)])
            before_step()
        before_step()
        n = run_episodes(states, eps, goals, on_step=on_step)
        return [n, steps]
    plain, got = _in_a_backlogged_stream(scenario)
    assert all(c >= 1 for c in plain[0]) and [len(s) for s in plain[1]] == [2] * 9 + [1] * 3
    for i, (a, b) in enumerate(zip(got[1], plain[1])):
        sc.assert_same(a, b, f"step {i}")
    assert got[0] == plain[0]

