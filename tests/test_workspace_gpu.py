"""No result of the library depends on what its device memory held before the call.

Every other GPU test builds a handle, calls it on well-formed input and compares the output; a kernel that reads a padded row, an
unwritten split-K slot, a capacity row past ``count[b]`` or an index list it did not fill passes all of them, because a fresh
process's allocations are almost always zeros.  Here every case follows one protocol:

  (a) ``r0``: a fresh handle with plain options on a good input;
  (b) a fresh handle under ``poisoned()`` -- library option ``debug_poison_alloc``: every device allocation the library makes for
      itself starts as 0xFF bytes (NaN as fp32 / fp64, -1 as int, all ones as a key) -- gives ``same(r, r0)``;
  (c) on ONE handle a history of other calls (all-NaN and all-inf inputs, other batch sizes and map sizes that regrow and re-lay
      the arena, range errors of the fp16x3 mode) and then the good input again gives ``same(r, r0)`` -- on the plain handle and on
      the poisoned one;
  (d) where a committed golden exists for the input, ``r0`` is within the tolerance the test that owns that golden asserts
      (imported, not restated).

``same`` is bit equality (tests/workspace_cases.py); the ``torch.empty`` outputs of the Python mirrors are served from 0xFF-filled
blocks (``dirty_torch_cache``).  The values themselves are pinned by the existing tests of the same cases (F.conv2d, the oracles,
the goldens); this module pins independence from history, so it needs no reference of its own.

Integer buffers: the poison turns a latent read-before-write of an index into a read at -1.  Before this module first ran, every
integer buffer was checked by reading -- producer, then what bounds each consumer:

  csrc/rcnn_post.hip
  sel_idx, sel_score   rpn_topk_kernel<false>: k[l] entries per level = all Ktot; or rpn_rank_select_kernel: ranks 0 .. k[l]-1 of
                       distinct keys, each once                          | rpn_decode_kernel: j < Ktot
  cand                 rpn_topk_kernel<true>: ks entries per slice       | rpn_rank_select_kernel: lvl_cnt[l] = the sum of those ks
  ckey, cbox, ccat     rpn_decode_kernel: every j < Ktot (ckey: all Kpad) | sorts: Kpad / Ktot; level NMS: k[l]; gather: the j inside a key
  ckey_sorted          rank_sort_keys_kernel: ranks < nvalid[b]          | gather_sorted_kernel: r < nvalid[b], else key 0
  sbox, scat, sscore   gather_sorted_kernel: all B * Ktot rows           | NMS, compaction: rows < nvalid[b]
  nvalid, dnvalid      the sort kernels: every image                     | gather, NMS, scan, compaction
  nms_ws               mask kernels: words of column blocks >= the row's | scans: the diagonal word and words right of it, rows < n
  keep, keepl, dkeep   nms_scan_dev_kernel: i < n (zeros after an early stop) | compaction: r < n; level form: j - koff[l] < k[l]
  lvl_count            synchronous upload when (B, k[]) changes          | the level scans
  prop_count, roi_level, rois   the compaction kernels: every image, all cap rows (empty rois past the count) | box_post, ROIAlign
  dkeys                zeroed by the compaction kernels, box_post_kernel's appends | sort_keys_counted_kernel
  dkey, dbox, dcat     box_post_kernel: the dkeys[b] appended keys, boxes / classes of rois < prop_count[b] | counted sort: i < dkeys[b];
                       gather: the candidate index inside a key
  det_*, det_count     compact_dets_kernel: rows < det_count[b], every image | pack_dets_kernel: the host offsets made of det_count
  mlevel, mrois        pack_dets_kernel: i < n                           | ROIAlign: n
  range_flag           hipMemsetAsync per call                            | atomicOr, the host read
  csrc/goal.hip
  active (4 flag arrays)  hipMemsetAsync / fmm_flags_clear_batch_kernel per solve, fmm_init marks the seed tiles | the round kernels
  counters             hipMemsetAsync before every batch of rounds         | host: the rounds of that batch, unsettled episodes only
  maxbits, results     hipMemsetAsync per use                              | atomicMax, goal_weight
  partial, out_idx, out_val, sum, wt_part   written in full by the kernel before their reader in the same call
  wt_last              the copy after a select that did not keep the last weights | read only when the host's have_last is set
  csrc/mapping.hip
  keys, pos, coords    every point, every frame                            | all later kernels of the frame
  cell_head / cnt / fill / first, cursor, stats, proj   initialised at create / reserve AFTER the fill, re-armed by map_finish
  seg                  map_fill_kernel: [cell_head, cell_head + cell_cnt)  | map_place_kernel: the same range
  skey                 map_place_kernel: every slot (a point's key, or INVALID behind the cursor) | map_voxels_kernel
  sidx                 written, never read

No consumer reads an entry the same call did not write; nothing had to be fixed.

Shown to bite with mutants built aside (values only, no address changed): with nchw_to_nhwc_pad_kernel leaving the pad channels
unwritten, every prediction case of this module fails with NaN logits while tests/test_pred_gpu.py passes; without the per-call
reset of the detector's range flag, the fp16x3 detector cases fail with a spurious range error while the existing fp16x3 detector
tests pass.  Dropping the hipMemsetAsync of peanut_nms_segments changes nothing anywhere: its scan reads only the words its mask
kernel wrote (test_nms_bit_matrix_workspace), and the detector runs the device-count NMS of rcnn_post.hip, which has no memset.
"""
import contextlib
import os
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import test_conv_gpu as tc
import test_goal_gpu as tg
import test_mapping_batch_gpu as tmb
import test_mapping_edges_gpu as tme
import test_pred_gpu as tp
import test_rcnn_selection_gpu as trs
from workspace_cases import dirty_torch_cache, first_difference, poisoned, same

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")


def _assert_same(got, want, what):
    assert same(got, want), f"{what}: {first_difference(got, want)}"


def _contexts():
    """(name, context) of the two handle kinds every history runs on."""
    return [("plain", contextlib.nullcontext()), ("poisoned", poisoned())]


# =====================================================================================================================
# Prediction forward
# =====================================================================================================================
PRED_MODELS = {
    "fp32": {},
    "direct": dict(conv_algo="direct"),
    "unfolded": dict(fold_ppm=False),
    "bf16x6": dict(precision="bf16x6"),
    "fp16x3": dict(precision="fp16x3"),
}
# the tolerances of the tests that own pspnet_golden.npz: TOL for the fp32 forms (test_golden_vectors), the parameter table of
# test_split_precision_forward_within_contract for the emulated modes
_EMULATED_TOL = dict(tp.test_split_precision_forward_within_contract.pytestmark[0].args[1])
PRED_INPUTS = ["odd_100", "rect_72x104", "b3_64x64"]
BIG_MAP = (1, 200, 200)          # grows the arena and lays it out differently

_pred_sd = {}


def _pred_model(**kw):
    from peanut_amd.prediction import PEANUT_Prediction_Model
    from peanut_amd.weights import PredCfg, make_seeded_state_dict
    if not _pred_sd:
        cfg = PredCfg()
        _pred_sd["cfg"], _pred_sd["sd"] = cfg, make_seeded_state_dict(cfg, seed=0)
    return PEANUT_Prediction_Model(SimpleNamespace(sem_gpu_id=0), state_dict=_pred_sd["sd"], cfg=_pred_sd["cfg"], **kw)


def _pred_input(name, golden_dir):
    """-> (input on the device, golden logits or None)."""
    if name == "b3_64x64":
        return tp._inputs(3, 14, 64, 64, seed=64 * 1000 + 64).cuda(), None
    z = np.load(os.path.join(golden_dir, "pspnet_golden.npz"))
    assert int(z[f"{name}/c_in"]) == 14 and int(z[f"{name}/weight_seed"]) == 0
    return torch.from_numpy(z[f"{name}/input"].astype(np.float32)).cuda(), torch.from_numpy(z[f"{name}/logits"])


def _pred_call(m, x):
    """The logits of ``x`` behind the host-facing range check (fp16x3: FloatingPointError instead of NaN logits), written into a
    ``torch.empty`` block that held 0xFF."""
    dirty_torch_cache(x.shape[0] * 6 * x.shape[2] * x.shape[3] * 4)
    return m.model.check_range(m.get_prediction_batch(x, apply_sigmoid=False))


def _pred_bad(m, x, raises, must_be_nonfinite=True):
    """A call that poisons the arena: it raises in fp16x3 and returns non-finite logits in the other modes."""
    if raises:
        with pytest.raises(FloatingPointError, match="fp16x3"):
            _pred_call(m, x)
    else:
        y = _pred_call(m, x)
        if must_be_nonfinite:
            assert not bool(torch.isfinite(y).all()), "the non-finite input did not reach the output"


def _pred_history(m, x, r0, raises, who):
    """good, NaN at the same shape, good, NaN at BIG_MAP, +inf at the first shape, good, the fp16 overflow x * 3e6, good."""
    nan_big = torch.full((BIG_MAP[0], x.shape[1]) + BIG_MAP[1:], NAN, device="cuda")
    _assert_same(_pred_call(m, x), r0, f"{who}: first call")
    _pred_bad(m, torch.full_like(x, NAN), raises)
    _assert_same(_pred_call(m, x), r0, f"{who}: after an all-NaN input")
    _pred_bad(m, nan_big, raises)
    _pred_bad(m, torch.full_like(x, INF), raises)
    _assert_same(_pred_call(m, x), r0, f"{who}: after NaN at {BIG_MAP} and +inf")
    _pred_bad(m, x * 3.0e6, raises, must_be_nonfinite=False)
    _assert_same(_pred_call(m, x), r0, f"{who}: after the fp16 overflow input")


@pytest.mark.parametrize("inp", PRED_INPUTS)
@pytest.mark.parametrize("model", list(PRED_MODELS))
def test_prediction_forward(model, inp, golden_dir):
    """odd_100: B = 1, 13 x 13 feature map -- overlapping pyramid bins, overhanging Winograd tiles, the grouped PSP path with padded
    rows on the skinny GEMM (asserted by name for the default model); rect_72x104: 9 x 13 at B = 2; 3 x 64 x 64."""
    kw = PRED_MODELS[model]
    raises = kw.get("precision") == "fp16x3"
    x, golden = _pred_input(inp, golden_dir)
    plain = _pred_model(**kw)
    r0 = _pred_call(plain, x)                                            # (a)
    if golden is not None:                                               # (d)
        err = float((r0.cpu() - golden).abs().max())
        tol = _EMULATED_TOL.get(kw.get("precision"), tp.TOL)
        print(f"{model} {inp}: max-abs against the golden {err:.3e} (asserted {tol})")
        assert err <= tol
    with poisoned():                                                     # (b), with a shape switch, then (c) on the poisoned handle
        p = _pred_model(**kw)
        _assert_same(_pred_call(p, x), r0, "poisoned handle")
        big = tp._inputs(BIG_MAP[0], x.shape[1], BIG_MAP[1], BIG_MAP[2], seed=200).cuda()
        assert bool(torch.isfinite(_pred_call(p, big)).all())
        _assert_same(_pred_call(p, x), r0, f"poisoned handle after a {BIG_MAP} map")
        _pred_history(p, x, r0, raises, "poisoned handle")
        del p
    _pred_history(plain, x, r0, raises, "plain handle")                  # (c)
    if model == "fp32" and inp == "odd_100":
        fam = {n: k for n, k, *_ in plain.model.profile(x)}
        pyramid = [k for n, k in fam.items() if "psp_modules" in n or "bottleneck.conv[ppm" in n]
        assert pyramid and all(k == "gemm_skinny" for k in pyramid), pyramid
        _assert_same(_pred_call(plain, x), r0, "plain handle after profile()")


def test_prediction_auto_precision_after_the_escalation(golden_dir):
    """precision='auto' on a poisoned handle: the good input, the overflowing one (announced escalation to bf16x6: a second handle,
    created and first used with the fp16x3 handle's arena full of NaN next to it), the good input again -- the last result is a
    fresh bf16x6 model's (the documented use: INTEGRATION.md)."""
    x, _ = _pred_input("odd_100", golden_dir)
    want = _pred_call(_pred_model(precision="bf16x6"), x)
    with poisoned():
        m = _pred_model(precision="auto")
        assert bool(torch.isfinite(_pred_call(m, x)).all()) and m.model.precision == "fp16x3"
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            y = _pred_call(m, x * 3.0e6)
        assert any("bf16x6" in str(i.message) for i in w) and m.model.precision == "bf16x6"
        assert bool(torch.isfinite(y).all())
        _assert_same(_pred_call(m, x), want, "after the escalation")


def test_prediction_graph_mode_across_an_arena_regrowth():
    """Graph mode on a side stream (as test_graph_replay_is_bit_identical): S three times -- direct, captured, replayed -- then NaN
    at BIG_MAP, which frees the arena and the captured graphs, then S three times again; every result is the plain handle's."""
    x = tp._inputs(2, 14, 72, 104, seed=5).cuda()
    r0 = _pred_model().get_prediction_batch(x, apply_sigmoid=True)
    nan_big = torch.full((BIG_MAP[0], 14) + BIG_MAP[1:], NAN, device="cuda")
    for who, ctx in _contexts():
        with ctx:
            g = _pred_model()
            g.model.use_graph(True)
            side = torch.cuda.Stream()
            out, out_big = torch.empty_like(r0), torch.empty((BIG_MAP[0], 6) + BIG_MAP[1:], device="cuda")
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                for part in ("before", "after"):
                    for rep in range(3):
                        out.fill_(NAN)
                        g.get_prediction_batch(x, apply_sigmoid=True, out=out)
                        side.synchronize()
                        _assert_same(out, r0, f"{who}: {part} the regrowth, call {rep}")
                    if part == "before":
                        g.get_prediction_batch(nan_big, apply_sigmoid=True, out=out_big)
                        side.synchronize()
                        assert bool(torch.isnan(out_big).all())
            torch.cuda.synchronize()
            del g


# =====================================================================================================================
# Single convs, one case per kernel family (the cases and option sets of tests/test_conv_gpu.py, which holds them to F.conv2d)
# =====================================================================================================================
def _conv_protocol(make, B, B2, H, W, c1, c2=0, residual=False, want=None, prefix=None):
    """good; x, x2 and residual all NaN; good; NaN at batch B2 (another split plan; regrown Winograd scratch); good -- on a plain
    and on a poisoned handle, every good result equal to the first one of the plain handle.  ``want`` / ``prefix``: the kernel
    family every good call must report."""
    def args(b, nan):
        g = torch.Generator(device="cuda").manual_seed(1000 * b + H)

        def mk(shape):
            return torch.full(shape, NAN, device="cuda") if nan else torch.randn(shape, device="cuda", generator=g)
        ho, wo = plain.out_hw(H, W)
        return mk((b, H, W, c1)), (mk((b, H, W, c2)) if c2 else None), (mk((b, ho, wo, plain.cout)) if residual else None)

    def call(conv, a):
        ho, wo = conv.out_hw(H, W)
        dirty_torch_cache(a[0].shape[0] * ho * wo * conv.cout * 4)
        return conv(a[0], x2=a[1], residual=a[2])

    def good_call(conv, what):
        y = call(conv, good)
        fam = tc._last_kernel()
        if want is not None:
            assert fam == want, (what, fam)
        if prefix is not None:
            assert fam.startswith(prefix), (what, fam)
        return y, fam

    plain = make()
    good, nan, nan2 = args(B, False), args(B, True), args(B2, True)
    r0, fam0 = good_call(plain, "fresh plain handle")                    # (a)
    assert bool(torch.isfinite(r0).all())
    print(f"kernel family {fam0}")
    for who, ctx in _contexts():
        with ctx:
            conv = plain if who == "plain" else make()
            y, fam = good_call(conv, f"{who}: first call")               # (b) on the poisoned handle
            assert fam == fam0
            _assert_same(y, r0, f"{who}: first call")
            assert bool(torch.isnan(call(conv, nan)).all())
            _assert_same(good_call(conv, who)[0], r0, f"{who}: after an all-NaN call")
            assert bool(torch.isnan(call(conv, nan2)).all())
            _assert_same(good_call(conv, who)[0], r0, f"{who}: after an all-NaN call at batch {B2}")   # (c)


def _pw(case_or_hw, options=None, precision="fp32", **kw):
    """A factory of FusedConv handles for a pointwise case (B, H, W, cin, cout, stride, relu, residual) of test_conv_gpu.py."""
    from peanut_amd.ops import FusedConv
    _, _, _, cin, cout, stride, relu, _ = case_or_hw
    g = torch.Generator().manual_seed(sum(case_or_hw[:6]))
    w = tc._rand((cout, cin, 1, 1), g, (2.0 / cin) ** 0.5)
    scale, shift = torch.rand(cout, generator=g) + 0.5, tc._rand((cout,), g, 0.1)
    return lambda: FusedConv(w, scale, shift, stride=stride, relu=relu, precision=precision, options=options, **kw)


def _conv3(cin, cout, dil, relu, options=None, precision="fp32", conv_algo="auto", stride=1):
    from peanut_amd.ops import FusedConv
    g = torch.Generator().manual_seed(cin + cout + dil)
    w = tc._rand((cout, cin, 3, 3), g, (2.0 / (cin * 9)) ** 0.5)
    scale, shift = torch.rand(cout, generator=g) + 0.5, tc._rand((cout,), g, 0.1)
    return lambda: FusedConv(w, scale, shift, stride=stride, padding=dil, dilation=dil, relu=relu, precision=precision,
                             conv_algo=conv_algo, options=options)


def test_conv_igemm_tail_split_k_dilation_4():
    case = tc.CASES[8]
    B, H, W, cin, cout, k, s, p, d, relu, residual = case
    assert (k, d, cin, cout) == (3, 4, 512, 512)
    _conv_protocol(_conv3(cin, cout, d, relu, conv_algo="direct"), B, 2, H, W, cin, residual=residual, prefix="conv_igemm_")


def test_conv_pw_two_sources_128x128():
    from peanut_amd.ops import FusedConv
    B, H, W, c1, c2, cout = 1, 23, 17, 256, 512, 1024          # test_pointwise_two_source_matches_torch: ragged M, few tiles, split-K
    g = torch.Generator().manual_seed(B + H + W + c1 + c2 + cout)
    w = tc._rand((cout, c1 + c2, 1, 1), g, (2.0 / (c1 + c2)) ** 0.5)
    scale, shift = torch.rand(cout, generator=g) + 0.5, tc._rand((cout,), g, 0.1)
    _conv_protocol(lambda: FusedConv(w, scale, shift, relu=True), B, 2, H, W, c1, c2=c2, want="conv_pw_glds_128x128")


def test_conv_pw256p_stream_k_tail():
    case = (13, 64, 64, 512, 256, 1, True, False)               # test_pw256p_stream_k_tail: 416 tiles, 160 tail tiles in runs of 10
    _conv_protocol(_pw(case, options=tc.P256P_OPTS), case[0], 11, case[1], case[2], case[3], residual=case[7],
                   want="conv_pw_glds_256x128p")


def test_conv_pw256wp():
    case = tc.WP_CASES[5]                                       # 32 tiles < CUs: nothing but raw partial tiles + the reduce
    assert case[:5] == (2, 64, 64, 512, 256)
    _conv_protocol(_pw(case, options=tc.WP_OPTS), case[0], 3, case[1], case[2], case[3], residual=case[7], want="conv_pw_glds_256x256p")


def test_conv_pw_ares():
    case = tc.ARES_CASES[2]                                     # K = 128, residual
    assert case[:5] == (8, 64, 64, 128, 512)
    _conv_protocol(_pw(case), case[0], 5, case[1], case[2], case[3], residual=case[7], want="conv_pw_ares_128x128")


def test_conv_patch():
    B, H, W, cin, cout, s, relu, family = tc.PATCH_CASES[4]     # ragged both ways
    _conv_protocol(_conv3(cin, cout, 1, relu, options={"patch_mintiles": 1}, conv_algo="direct", stride=s), B, 3, H, W, cin, want=family)


@pytest.mark.parametrize("tile", [4, 6])
def test_conv_winograd_overhanging_tiles(tile):
    """(1, 15, 13, 256, 320): tiles overhang the map on both axes, cout is no tile multiple; batch 3 regrows V and M."""
    B, H, W, cin, cout, d, relu, residual = tc.WINO_CASES[1]
    make = _conv3(cin, cout, d, relu, options={"wino_m": tile})
    _conv_protocol(make, B, 3, H, W, cin, residual=residual)
    x = torch.randn((B, H, W, cin), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    res = torch.zeros((B, H, W, cout), device="cuda")
    direct = _conv3(cin, cout, d, relu, conv_algo="direct")()
    assert not torch.equal(make()(x, residual=res), direct(x, residual=res))      # the Winograd path did run


_RS_GEMMS = [tc.RS_CASES[1], tc.RS_CASES[3], tc.RS_CASES[14]]   # 64x64 ragged M; 128x128 split-K over 128 k-tiles; 256x256 split-K tail


@pytest.mark.parametrize("precision", ["bf16x6", "fp16x3"])
@pytest.mark.parametrize("case,family", _RS_GEMMS, ids=[f for _, f in _RS_GEMMS])
def test_conv_register_split_gemm(case, family, precision):
    assert [f for _, f in _RS_GEMMS] == ["64x64", "128x128", "256x256"]
    _conv_protocol(_pw(case, precision=precision), case[0], case[0] + 1, case[1], case[2], case[3], residual=case[7],
                   want="gemm_" + tc.RS_TAG[precision] + family)


@pytest.mark.parametrize("precision", ["bf16x6", "fp16x3"])
def test_conv_register_split_conv(precision):
    B, H, W, cin, cout, k, s, p, d, relu, residual = tc.CASES[8]
    _conv_protocol(_conv3(cin, cout, d, relu, precision=precision, conv_algo="direct"), B, 2, H, W, cin,
                   want="conv_" + tc.RS_TAG[precision] + "128x128")


def test_nms_bit_matrix_workspace():
    """peanut_nms_segments on a workspace that held 0xFF: rows of the bit matrix carry words for the columns of their own block and
    later ones only, and the scan reads no others."""
    from peanut_amd.rcnn import nms_keep_segments
    g = torch.Generator().manual_seed(9)
    counts = [130, 0, 70, 257]
    n = sum(counts)
    ctr, size = torch.rand((n, 2), generator=g) * 100.0, torch.rand((n, 2), generator=g) * 30.0 + 10.0
    boxes = torch.cat([ctr - size / 2, ctr + size / 2], 1).cuda()
    cats = torch.randint(0, 3, (n,), generator=g).cuda()
    sizes = [sum(k * ((k + 63) // 64) * 8 for k in counts), n]

    def fill(byte):
        blocks = [torch.full((s,), byte, dtype=torch.uint8, device="cuda") for s in sizes]
        torch.cuda.synchronize()
        del blocks
    fill(0)
    r0 = nms_keep_segments(boxes, cats, counts, 0.5)
    assert 0 < int(r0.sum()) < n
    fill(0xFF)
    _assert_same(nms_keep_segments(boxes, cats, counts, 0.5), r0, "workspace of 0xFF bytes")


# =====================================================================================================================
# Detector.  Frames are uint8: the detector cannot be poisoned through its input, so step (b) is the main instrument.
# =====================================================================================================================
DET_FORMS = {
    "default": {},
    # rcnn_rpn_fused, rcnn_rank_sort, rcnn_topk_slice and rcnn_nms_levels all at their non-default values
    "round4_unfused": {**trs.FORMS["round4"], "rcnn_rpn_fused": 0},
}
assert "round4" in trs.ALL_FORMS and set(trs.FORMS["round4"]) == {"rcnn_topk_slice", "rcnn_rank_sort", "rcnn_nms_levels"}


def _det_case(name):
    from rcnn_cases import make_case, small_inputs
    cfg, sd, img = small_inputs() if name == "small" else make_case(name)
    return cfg, sd, img.cuda()


def _det_net(cfg, sd, form, precision):
    from peanut_amd import _lib
    from peanut_amd.rcnn import MaskRCNN
    with _lib.default_options(**DET_FORMS[form]):
        return MaskRCNN(cfg, sd, precision=precision)


def _det_run(net, cfg, img):
    """Everything ``inference`` and ``semantic`` return: boxes, scores, classes, masks per image, the category map, the counts."""
    B, H, W = img.shape[:3]
    D, K = cfg.detections_per_image, cfg.num_classes
    outs = [B * D * 16, B * D * 4, B * D * 4]
    dirty_torch_cache(outs + [B * D * H * W])
    inst = net.inference(img)
    dirty_torch_cache(outs + [B * H * W * (K + 1) * 4])
    sem = net.semantic(img, K, 0.0, 0.0, None)
    return dict(instances=inst, semantic=sem, counts=list(net.last_detection_counts))


@pytest.mark.parametrize("form", list(DET_FORMS))
@pytest.mark.parametrize("case,precision", [("small", "fp32"), ("small", "fp16x3"), ("all_tied", "fp32"), ("no_proposal", "fp32")])
def test_detector_on_a_poisoned_handle(case, precision, form):
    """small: R-50, two 96 x 128 frames, in fp32 and in fp16x3 (whose range scan covers whole stage buffers: no spurious range
    error); all_tied and no_proposal (tests/rcnn_cases.py): full tie runs and empty lists are where a stale key or count decides."""
    cfg, sd, img = _det_case(case)
    r0 = _det_run(_det_net(cfg, sd, form, precision), cfg, img)          # (a)
    n = [len(i["scores"]) for i in r0["instances"]]
    print(f"{case} {precision} {form}: detections {n}")
    assert (sum(n) == 0) == (case == "no_proposal") and r0["counts"] == n
    with poisoned():                                                     # (b)
        net = _det_net(cfg, sd, form, precision)
        _assert_same(_det_run(net, cfg, img), r0, "poisoned handle")
        _assert_same(_det_run(net, cfg, img), r0, "poisoned handle, second call")


@pytest.mark.parametrize("precision", ["fp32", "fp16x3"])
def test_detector_history(precision):
    """The two frames; one 120 x 90 frame at B = 1 (other level sizes, other capacities of every stage buffer); the two frames."""
    cfg, sd, img = _det_case("small")
    other = torch.randint(0, 256, (1, 120, 90, 3), generator=torch.Generator().manual_seed(12), dtype=torch.uint8).cuda()
    r0 = _det_run(_det_net(cfg, sd, "default", precision), cfg, img)
    other0 = _det_run(_det_net(cfg, sd, "default", precision), cfg, other)
    for who, ctx in _contexts():
        with ctx:
            net = _det_net(cfg, sd, "default", precision)
            _assert_same(_det_run(net, cfg, img), r0, f"{who}: first call")
            _assert_same(_det_run(net, cfg, other), other0, f"{who}: the 120 x 90 frame")
            _assert_same(_det_run(net, cfg, img), r0, f"{who}: the two frames again")          # (c)


# =====================================================================================================================
# Map projection (no NaN observations: tests/test_mapping_edges_gpu.py explains why)
# =====================================================================================================================
def _golden_frames(golden_dir, name, n=3):
    z = np.load(os.path.join(golden_dir, "mapping_golden.npz"))
    obs = np.zeros((n, 14, 120, 160), np.float32)
    obs[:, 3] = z[f"{name}/depth"][:n]
    obs[:, 4:] = z[f"{name}/sem"][:n].astype(np.float32)
    return torch.from_numpy(obs).cuda(), torch.from_numpy(z[f"{name}/pose_obs"][:n]).cuda(), z


def _map_run(sm, obs, rel):
    """Every frame from an empty map: per frame (fp_map_pred, map, pose)."""
    maps, pose, rec = torch.zeros(14, 480, 480, device="cuda"), torch.tensor([12.0, 12.0, 0.0], device="cuda"), []
    for i in range(obs.shape[0]):
        dirty_torch_cache([100 * 100 * 4, 14 * 480 * 480 * 4])
        fp, maps, _, _ = sm(obs[i:i + 1], rel[i], maps, pose, None)
        rec.append((fp.clone(), maps, pose.clone()))
    return rec


def test_map_projection_on_a_poisoned_handle(golden_dir):
    """The first three frames of the golden sequence seq0, single: bit-equal to the unpoisoned handle's, whose fp_map_pred and
    poses are the golden's (gates of test_golden_sequences)."""
    obs, rel, z = _golden_frames(golden_dir, "seq0")
    r0 = _map_run(tmb._module(tmb._args()), obs, rel)                    # (a)
    for i, (fp, _, pose) in enumerate(r0):                               # (d)
        assert np.array_equal(np.packbits(fp.cpu().numpy().astype(bool)), z["seq0/fp_map_bits"][i]), f"frame {i}: fp_map_pred"
        assert float(np.abs(pose.cpu().numpy() - z["seq0/poses"][i]).max()) <= tme.POSE_TOL
    assert float(r0[-1][1][4:].sum()) > 0
    with poisoned():                                                     # (b)
        _assert_same(_map_run(tmb._module(tmb._args()), obs, rel), r0, "poisoned handle")


def test_map_projection_batch_on_a_poisoned_handle(golden_dir):
    """The same as E = 4 through peanut_map_reserve / forward_batch: seq0, seq1, seq0 from its fourth frame, seq1 from its third."""
    a, ra, _ = _golden_frames(golden_dir, "seq0", 6)
    b, rb, _ = _golden_frames(golden_dir, "seq1", 5)
    episodes = [(a[:3], ra[:3]), (b[:3], rb[:3]), (a[3:6], ra[3:6]), (b[2:5], rb[2:5])]

    def run(sm):
        maps = [torch.zeros(14, 480, 480, device="cuda") for _ in range(4)]
        poses, rec = torch.tensor([[12.0, 12.0, 0.0]] * 4, device="cuda"), []
        for i in range(3):
            dirty_torch_cache([4 * 100 * 100 * 4] + [14 * 480 * 480 * 4] * 4)
            fp, maps, _, _ = sm.forward_batch(torch.stack([e[0][i] for e in episodes]), torch.stack([e[1][i] for e in episodes]), maps, poses)
            rec.append((fp.clone(), list(maps), poses.clone()))
        return rec
    r0 = run(tmb._module(tmb._args(), reserve=4))
    single = _map_run(tmb._module(tmb._args()), *episodes[0])
    for i in range(3):      # slot 0 is the single-episode run (what test_mapping_batch_gpu.py holds for every slot)
        _assert_same((r0[i][0][0:1], r0[i][1][0], r0[i][2][0]), single[i], f"frame {i}, slot 0 against the single run")
    with poisoned():
        _assert_same(run(tmb._module(tmb._args(), reserve=4)), r0, "poisoned handle")


def test_map_projection_history():
    """On one handle: the densest frame of the dense-cell edge scene (2352 points in a cell), an empty frame, then the tested
    frame -- against a fresh handle's result for the tested frame."""
    from oracle import mapping_scenes
    frames = [mapping_scenes.dense_frame(10.0, 3), mapping_scenes.far_frame(), mapping_scenes.make_sequence(30, 1)[0]]
    obs = torch.from_numpy(np.stack([mapping_scenes.frame_to_obs(f) for f in frames])).cuda()
    rel = torch.from_numpy(np.stack([f["pose"] for f in frames]).astype(np.float32)).cuda()
    r0 = _map_run(tmb._module(tmb._args()), obs[2:3], rel[2:3])          # (a)
    assert float(r0[0][1][4:].sum()) > 0
    for who, ctx in _contexts():
        with ctx:
            sm = tmb._module(tmb._args())
            _map_run(sm, obs[0:2], rel[0:2])
            _assert_same(_map_run(sm, obs[2:3], rel[2:3]), r0, f"{who}: after the dense and the empty frame")      # (c)


# =====================================================================================================================
# Goal selection
# =====================================================================================================================
def _goal_inputs(h, w, seed, lmb):
    obst = tg._obstacles(h, w, seed).cuda()
    col = torch.zeros((h, w), dtype=torch.uint8)
    col[h // 2, w // 4:w // 2] = 1
    tps = [torch.rand((lmb[1] - lmb[0], lmb[3] - lmb[2]), generator=torch.Generator().manual_seed(seed + k)).cuda() for k in range(2)]
    return obst, col.cuda(), tps


def _select(sol, obst, col, lmb, loc, tp, temperature):
    dirty_torch_cache([sol.H * sol.W * 8, (lmb[1] - lmb[0]) * (lmb[3] - lmb[2]) * 8])
    return sol.select(obst, col, None, lmb, loc, tp, temperature, 5, want_dist=True, want_value=True)


@pytest.mark.parametrize("shape,seed,lmb,loc", [((64, 40), 4, (8, 56, 4, 36), (20, 15)), ((250, 333), 3, (20, 220, 40, 300), (100, 130))],
                         ids=["64x40", "250x333"])
def test_goal_select_on_a_poisoned_handle(shape, seed, lmb, loc):
    """Field, value map (target_pred * weights), goal, sum of the weights, keep-last flag, rounds and pass count of two selects in a
    row (the second reads the weights the first one left) at temperature 500, and of one at temperature 1, where the weights
    underflow and the last ones are kept."""
    from peanut_amd.goal import GeodesicSolver
    h, w = shape
    obst, col, tps = _goal_inputs(h, w, seed, lmb)

    def run():
        sol = GeodesicSolver(h, w, 2)
        return [_select(sol, obst, col, lmb, loc, tps[0], 500.0), _select(sol, obst, col, lmb, loc, tps[1], 500.0),
                _select(sol, obst, col, lmb, loc, tps[1], 1.0)]
    r0 = run()                                                           # (a)
    assert all(r["converged"] for r in r0) and bool(torch.isfinite(r0[0]["dist"]).any())
    with poisoned():                                                     # (b)
        _assert_same(run(), r0, "poisoned handles")


def test_goal_select_batch_on_poisoned_handles():
    from peanut_amd.goal import GeodesicSolver, select_batch
    h, w, lmb = 250, 333, (20, 220, 40, 300)
    inputs = [_goal_inputs(h, w, 30 + e, lmb) for e in range(3)]
    items = [(obst, col, None, lmb, (100 + 10 * e, 130 - 20 * e)) for e, (obst, col, _) in enumerate(inputs)]

    def run():
        sols = [GeodesicSolver(h, w, 2) for _ in range(3)]
        out = []
        for k in range(2):
            dirty_torch_cache([h * w * 8] * 3 + [(lmb[1] - lmb[0]) * (lmb[3] - lmb[2]) * 8] * 3)
            out.append(select_batch(sols, items, [tps[k] for _, _, tps in inputs], 500.0, 5, want_dist=True, want_value=True))
        return out
    r0 = run()
    with poisoned():
        _assert_same(run(), r0, "poisoned handles")
