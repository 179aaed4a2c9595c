"""The detector's selection kernels (csrc/rcnn_post.hip, the NMS / paste kernels of rcnn_ops.hip) on TIED and SATURATED
scores, through the unchanged C entries ``peanut_rcnn_inference`` / ``peanut_rcnn_semantic``.

Every other detector test feeds those kernels the scores of a seeded random-weight network, which are distinct by
construction (peanut_amd/rcnn_weights.py).  Here the state dicts are crafted (tests/rcnn_cases.py): zeroed head weights give
``0 * x + bias = bias`` bit for bit on the device and in the oracle, so both sides see the same logits and every decision --
which element is selected, in which order, how many -- is compared EXACTLY against oracle/rcnn_ref.py, stage by stage through
``debug_stage`` and in the returned instances.  The tie rule held on both sides: among equal scores the lower flat index first
("Ties in the detector's selections").  tests/test_oracles_cpu.py::test_crafted_selection_cases_have_the_properties_
they_are_named_for checks from the oracle alone that each case really has its ties / full capacities / empty lists.

Forms: the cases that pin the RPN selection run under the default options, the round-4 forms (one workgroup per level, bitonic
key sort, one score-sorted NMS list) and ``rcnn_topk_slice=300`` (a level's logits cut into up to eight slices; in the small
configuration every winner of a level lies in its first slice, at the deployed sizes -- full_capacities -- the cut falls in a
middle slice, which tests/test_oracles_cpu.py pins); cases 1 and 3 also under ``rcnn_nms_levels=0`` alone, the one form that
orders an image's candidates with rank_sort_keys_kernel.  Every form is held to the ORACLE, not to another form.

Scores of the bias-only cases are ``softmax(bias)``, the device's expf against glibc's.  The bound follows the rule "4 x the
measured max |device - oracle| over all_tied, saturated and full_capacities, or 1e-6, whichever is larger, never above the
suite's 1e-4".  SCORE_TOL = 1e-6 is that rule's floor, the strictest value it can yield: the scores of these cases are 1 / 10
and 1 / 1 (exp(0) = 1, and 1 + 9 e^-40 rounds to 1, on both sides), where a difference, if any, is an ulp or two of a value
<= 1 (6e-8 to 1.2e-7).  Every case prints its measured difference before it asserts."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SCORE_TOL = 1e-6

FORMS = {
    "default": {},
    "round4": dict(rcnn_topk_slice=0, rcnn_rank_sort=0, rcnn_nms_levels=0),
    "slice300": dict(rcnn_topk_slice=300),
    "ranksort": dict(rcnn_nms_levels=0),      # one list per image, ordered by counting: rank_sort_keys_kernel
}
ALL_FORMS = ["default", "round4", "slice300"]
TIE_FORMS = ALL_FORMS + ["ranksort"]          # cases 1 and 3 also reach the counting sort of the one-list form
ONE_LIST_FORMS = ("round4", "ranksort")       # rcnn_nms_levels=0: the forms that sort one list per image and write nvalid

_oracle_cache = {}


def _oracle(name):
    """(instances, stages) of a case; shared between its option-set variants (the oracle does not depend on device options)."""
    if name not in _oracle_cache:
        from rcnn_cases import oracle_run
        _oracle_cache[name] = oracle_run(name)
    return _oracle_cache[name]


def _device(name, form, precision="fp32"):
    from peanut_amd import _lib
    from peanut_amd.rcnn import MaskRCNN
    from rcnn_cases import make_case
    cfg, sd, img = make_case(name)
    with _lib.default_options(**FORMS[form]):
        net = MaskRCNN(cfg, sd, precision=precision)
    return net, cfg, img


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check_selection(net, cfg, img, stages, nan_scores=False):
    """sel_idx / sel_score: the per-level top-k, level after level, against the oracle's stable sort."""
    from rcnn_cases import level_ks
    B = img.shape[0]
    ktot = sum(k for _, k, _ in level_ks(cfg, img.shape[1], img.shape[2]))
    assert stages["sel_idx"].shape == (B, ktot)
    idx = net.debug_stage("sel_idx", (B, ktot), torch.int32).cpu().long()
    sc = net.debug_stage("sel_score", (B, ktot)).cpu()
    for off, k, _ in level_ks(cfg, img.shape[1], img.shape[2]):
        sl = slice(off, off + k)
        assert torch.equal(idx[:, sl], stages["sel_idx"][:, sl]), f"selected anchors of the level at offset {off} differ"
    ref = stages["sel_score"]
    if nan_scores:
        assert torch.equal(sc.isnan(), ref.isnan()) and bool(ref.isnan().any())
        sc, ref = torch.nan_to_num(sc, nan=0.0), torch.nan_to_num(ref, nan=0.0)
    assert torch.equal(_bits(sc), _bits(ref))


def _check_proposals(net, cfg, img, ref, stages, form, exact):
    """prop_count, nvalid (the forms that sort one list per image write it) and rois: the oracle's proposals in the oracle's
    order -- bit-equal (``exact``) or within 1e-3 px (test_proposals_from_oracle_logits' bound) -- and empty rows after them."""
    B, cap = img.shape[0], cfg.rpn_post_nms_topk
    cnt = net.debug_stage("prop_count", (B,), torch.int32).cpu().tolist()
    assert cnt == [len(r["proposals"]) for r in ref]
    if form in ONE_LIST_FORMS:
        assert net.debug_stage("nvalid", (B,), torch.int32).cpu().tolist() == stages["nvalid"]
    rois = net.debug_stage("rois", (B * cap, 5)).cpu()
    for b, r in enumerate(ref):
        n = len(r["proposals"])
        got = rois[b * cap:b * cap + n]
        assert torch.all(got[:, 0] == b)
        if exact:
            assert torch.equal(_bits(got[:, 1:]), _bits(r["proposals"])), f"image {b}: proposals are not bit-equal to the oracle's"
        elif n:
            assert (got[:, 1:] - r["proposals"]).abs().max().item() <= 1e-3
        if n < cap:
            assert float(rois[b * cap + n:(b + 1) * cap].abs().max()) == 0.0


def _edge_pixels(r, hw):
    """Pixels of an oracle instance list whose pasted value lies within 1e-6 of the mask threshold (either answer is right)."""
    from oracle import rcnn_ref
    vals = rcnn_ref.paste_values(r["mask_probs"], r["pred_boxes"], hw)
    return (vals - 0.5).abs() < 1e-6


def _check_exact_detections(net, cfg, got, ref, img):
    """Classes and order exact, boxes bit-equal, scores within SCORE_TOL, masks equal away from threshold-edge pixels -- in the
    stage buffers det_count / det_cls / det_score / det_out (per image, detections_per_image rows each) and in the returned
    instances."""
    B, H, W = img.shape[:3]
    D = cfg.detections_per_image
    assert len(got) == len(ref) == B
    assert net.debug_stage("det_count", (B,), torch.int32).cpu().tolist() == [len(r["scores"]) for r in ref]
    det_cls = net.debug_stage("det_cls", (B * D,), torch.int32).cpu()
    det_score = net.debug_stage("det_score", (B * D,)).cpu()
    det_out = net.debug_stage("det_out", (B * D, 4)).cpu()
    worst = 0.0
    for b, (g, r) in enumerate(zip(got, ref)):
        n = len(r["scores"])
        assert n > 0
        assert det_cls[b * D:b * D + n].tolist() == r["pred_classes"].tolist()
        assert torch.equal(_bits(det_out[b * D:b * D + n]), _bits(r["pred_boxes"]))
        assert g["pred_classes"].cpu().tolist() == r["pred_classes"].tolist()
        assert torch.equal(_bits(g["pred_boxes"].cpu()), _bits(r["pred_boxes"]))
        assert torch.equal(_bits(g["scores"].cpu()), _bits(det_score[b * D:b * D + n]))
        worst = max(worst, (g["scores"].cpu() - r["scores"]).abs().max().item())
        diff = g["pred_masks"].cpu() != r["pred_masks"]
        assert _edge_pixels(r, (H, W))[diff].all(), "mask differs away from the threshold"
        assert diff.float().mean().item() < 1e-4
    print(f"max |device - oracle| score: {worst:.3e}")
    assert worst <= SCORE_TOL


def _check_by_matcher(got, ref, need_saturated):
    """The matcher and tolerances of test_r101_batch16_full_proposals_against_the_vectorised_oracle (tests/rcnn_cases.py), plus:
    detections whose oracle scores are bit-equal keep the oracle's order."""
    from rcnn_cases import match_detections
    n_total = n_moved = 0
    worst_score = worst_box = 0.0
    worst_iou = 1.0
    for g, r in zip(got, ref):
        perm, moved, ws, wb, iou = match_detections(g, r)
        rs = r["scores"]
        same = _bits(rs)[:, None] == _bits(rs)[None, :]
        i, j = torch.nonzero(torch.triu(same, diagonal=1), as_tuple=True)
        assert bool((perm[i] < perm[j]).all()), "detections with bit-equal oracle scores came back in another order"
        n_total, n_moved = n_total + len(rs), n_moved + moved
        worst_score, worst_box, worst_iou = max(worst_score, ws), max(worst_box, wb), min(worst_iou, iou)
    sat = torch.cat([r["scores"] for r in ref])
    print(f"{n_total} detections ({n_moved} at another rank), max |score diff| {worst_score:.2e}, max |box diff| {worst_box:.2e} px, "
          f"min mask IoU {worst_iou:.4f}, oracle scores == 1.0: {int((sat == 1.0).sum())}")
    assert worst_score <= 1e-4 and worst_box <= 5e-2 and worst_iou >= 0.98 and n_moved <= n_total // 20
    if need_saturated:
        assert int((sat == 1.0).sum()) * 2 >= len(sat), "the case is not saturated any more"


# ---- 1, 2: RPN ties, the top-k cut inside a run of equal logits ----
@pytest.mark.parametrize("form", TIE_FORMS)
def test_rpn_ties_cut_inside_a_group(form):
    """Case 1.  Every objectness logit of anchor a is obj_bias[a] = (0.5, 2.0, -1.0) on all five levels: runs of h * w equal
    logits, k = 60 falls inside the run of 2.0 on the three fine levels and inside the run of -1.0 on the fourth, and equal scores
    meet across levels in the post-NMS top-k.  sel_idx equals the oracle's stable top-k, sel_score bit for bit, the proposals come
    in the oracle's order (seeded deltas: boxes within 1e-3 px)."""
    ref, stages = _oracle("rpn_ties")
    net, cfg, img = _device("rpn_ties", form)
    net.inference(img.cuda(), want_masks=False)
    _check_selection(net, cfg, img, stages)
    _check_proposals(net, cfg, img, ref, stages, form, exact=False)


@pytest.mark.parametrize("form", ALL_FORMS)
def test_rpn_ties_with_zero_deltas_gives_the_anchors_bit_for_bit(form):
    """Case 2.  The same logits with all anchor deltas zero (expf(0) = 1: the decode is exact): the proposals are anchors, and
    rois[:prop_count] is bit-equal to the oracle's proposals."""
    ref, stages = _oracle("rpn_ties_anchors")
    net, cfg, img = _device("rpn_ties_anchors", form)
    net.inference(img.cuda(), want_masks=False)
    _check_selection(net, cfg, img, stages)
    _check_proposals(net, cfg, img, ref, stages, form, exact=True)


# ---- 3: everything tied ----
@pytest.mark.parametrize("form", TIE_FORMS)
def test_everything_tied(form):
    """Case 3.  All logits 1.0, zero deltas, class bias zero (every class score of every proposal = 1 / 10 > 0.05: 9 x 40
    candidates tied), zero box regression, constant mask probability sigmoid(1).  The detection sort, the class-wise NMS and the
    10-detection cut work on ONE score: classes and order exact, boxes bit-equal, scores to SCORE_TOL, masks = the raster of the
    box (threshold-edge pixels excepted)."""
    ref, stages = _oracle("all_tied")
    net, cfg, img = _device("all_tied", form)
    got = net.inference(img.cuda())
    _check_selection(net, cfg, img, stages)
    _check_proposals(net, cfg, img, ref, stages, form, exact=True)
    _check_exact_detections(net, cfg, got, ref, img)


def test_everything_tied_through_the_semantic_entry():
    """Case 3 through peanut_rcnn_semantic: the category map equals the accumulation (segmentation.py:47-60) of the ORACLE's
    instances, away from pixels where one of them is within 1e-6 of the mask threshold."""
    from peanut_amd.segmentation import accumulate_instances
    ref, _ = _oracle("all_tied")
    net, cfg, img = _device("all_tied", "default")
    H, W = img.shape[1], img.shape[2]
    sem = net.semantic(img.cuda(), cfg.num_classes, 0.05, 0.05, None).cpu()
    assert net.last_detection_counts == [len(r["scores"]) for r in ref]
    for b, r in enumerate(ref):
        want = accumulate_instances(r["pred_masks"].cuda(), r["pred_classes"].cuda(), r["scores"].cuda(), cfg.num_classes, 0.05, 0.05, None).cpu()
        edges = _edge_pixels(r, (H, W))
        assert edges.float().mean().item() < 1e-4 and float(want.sum()) > 0
        edge = edges.any(0)
        assert torch.equal(sem[b][~edge], want[~edge])


# ---- 4, 5: saturated scores ----
def test_saturated_scores_keep_the_proposal_order():
    """Case 4.  Seeded RPN, class bias +40 on class 3, zero box regression: every score is exactly 1.0f on both sides, one class;
    the detections are the NMS survivors in PROPOSAL order (the stable rule: candidate index = proposal * K + class)."""
    ref, stages = _oracle("saturated")
    net, cfg, img = _device("saturated", "default")
    got = net.inference(img.cuda())
    B, cap, D = img.shape[0], cfg.rpn_post_nms_topk, cfg.detections_per_image
    _check_proposals(net, cfg, img, ref, stages, "default", exact=False)
    rois = net.debug_stage("rois", (B * cap, 5)).cpu()
    det_in = net.debug_stage("det_in", (B * D, 4)).cpu()
    worst = 0.0
    for b, (g, r) in enumerate(zip(got, ref)):
        n = len(r["scores"])
        assert n > 0 and len(g["scores"]) == n
        assert bool((r["scores"] == 1.0).all()) and bool((g["scores"].cpu() == 1.0).all())
        assert g["pred_classes"].cpu().tolist() == r["pred_classes"].tolist() == [3] * n
        assert (g["pred_boxes"].cpu() - r["pred_boxes"]).abs().max().item() <= 1e-3       # same survivors, same order
        worst = max(worst, (g["scores"].cpu() - r["scores"]).abs().max().item())
        # each detection's box at the network resolution is one of the image's proposals; their indices increase
        d = (det_in[b * D:b * D + n, None, :] - rois[None, b * cap:(b + 1) * cap, 1:]).abs().amax(2)
        assert float(d.min(1).values.max()) <= 1e-3
        src = d.argmin(1)
        assert bool((src[1:] > src[:-1]).all()), src.tolist()
    print(f"max |device - oracle| score: {worst:.3e}")
    assert worst <= SCORE_TOL


def test_saturated_scores_of_the_real_heads():
    """Case 5.  The seeded class-score weights times 60: the trained-network regime, most scores exactly 1.0 and the rest spread.
    Decisions rest on values that differ by rounding: the R-101 test's matcher and tolerances; at least half of the oracle's scores
    are exactly 1.0."""
    ref, stages = _oracle("saturated_real_heads")
    net, cfg, img = _device("saturated_real_heads", "default")
    got = net.inference(img.cuda())
    _check_proposals(net, cfg, img, ref, stages, "default", exact=False)
    _check_by_matcher(got, ref, need_saturated=True)


# ---- 6: select, then filter ----
@pytest.mark.parametrize("form", ALL_FORMS)
def test_top_k_is_taken_before_non_finite_boxes_are_dropped(form):
    """Case 6.  Case 1's logits, dx = inf on the best-scoring anchor: detectron2 takes the top-k first and drops non-finite boxes
    afterwards, so the selected anchors of the three fine levels are all dropped and only a handful of proposals per image is left
    (an implementation that filtered first would return 40).  prop_count, nvalid and rois exact (the surviving anchors have zero
    deltas)."""
    ref, stages = _oracle("select_then_filter")
    net, cfg, img = _device("select_then_filter", form)
    assert all(0 < len(r["proposals"]) < cfg.rpn_post_nms_topk // 2 for r in ref)
    net.inference(img.cuda(), want_masks=False)
    _check_selection(net, cfg, img, stages)
    _check_proposals(net, cfg, img, ref, stages, form, exact=True)


# ---- 7: no proposal at all ----
def test_no_valid_proposal_gives_empty_lists_and_a_zero_map():
    """Case 7.  dx = dy = 1e4 pushes every box out of the image (zero area after the clip): no proposal, no detection.  The
    proposal and box stages run at fixed capacity with device-side counts, so the C entry returns empty instance lists and an
    all-zero semantic map, without an error."""
    ref, stages = _oracle("no_proposal")
    assert [len(r["proposals"]) for r in ref] == [0, 0] and [len(r["scores"]) for r in ref] == [0, 0]
    net, cfg, img = _device("no_proposal", "default")
    B, H, W = img.shape[:3]
    got = net.inference(img.cuda())
    assert [len(g["scores"]) for g in got] == [0, 0]
    assert all(g["pred_masks"].shape == (0, H, W) and g["pred_boxes"].shape == (0, 4) for g in got)
    _check_proposals(net, cfg, img, ref, stages, "default", exact=True)
    assert net.debug_stage("det_count", (B,), torch.int32).cpu().tolist() == [0, 0]
    sem = net.semantic(img.cuda(), cfg.num_classes, 0.0, 0.0, None)
    assert sem.shape == (B, H, W, cfg.num_classes + 1) and float(sem.abs().max()) == 0.0
    assert net.last_detection_counts == [0, 0]


# ---- 8: the scale clamp ----
def test_scale_clamp_and_whole_frame_boxes():
    """Case 8.  dw = dh = 10 > log(1000 / 16): every box is clamped, then clipped to the whole frame; the NMS keeps one per level.
    prop_count exact, boxes within 1e-3 px, detections by the shared matcher."""
    ref, stages = _oracle("clamp")
    assert all(len(r["proposals"]) == 5 for r in ref)
    net, cfg, img = _device("clamp", "default")
    got = net.inference(img.cuda())
    _check_proposals(net, cfg, img, ref, stages, "default", exact=False)
    _check_by_matcher(got, ref, need_saturated=False)


# ---- 9: NaN objectness ----
@pytest.mark.parametrize("form", ALL_FORMS)
def test_nan_objectness_is_selected_then_dropped(form):
    """Case 9.  obj_bias = (0.5, NaN, -1.0), the quiet NaN with the sign bit clear: NaN ranks first in torch's descending sort and
    in ord_key, is selected, and is then dropped by the score validity test.  Counts and selected indices exact, boxes within
    1e-3 px (fp32; fp16x3 answers PEANUT_ERANGE by contract, below)."""
    ref, stages = _oracle("nan_objectness")
    net, cfg, img = _device("nan_objectness", form)
    assert all(0 < len(r["proposals"]) < cfg.rpn_post_nms_topk for r in ref)
    net.inference(img.cuda(), want_masks=False)
    _check_selection(net, cfg, img, stages, nan_scores=True)
    _check_proposals(net, cfg, img, ref, stages, form, exact=False)


def test_nan_objectness_in_fp16x3_is_a_range_error():
    from peanut_amd import _lib
    net, cfg, img = _device("nan_objectness", "default", precision="fp16x3")
    with pytest.raises(FloatingPointError, match="fp16x3") as e:
        net.inference(img.cuda())
    assert isinstance(e.value, _lib.PeanutRangeError)


# ---- 10, 11: the deployed selection sizes ----
@pytest.mark.parametrize("form", ALL_FORMS)
def test_capacities_exactly_full(form):
    """Case 10.  1000 / 1000 / 100 on one 480 x 640 frame, case 1's logits, zero deltas, class bias zero, zero box regression,
    constant masks: five levels x up to 1000 tied candidates with the cut inside a run on four levels, exactly 1000 proposals,
    exactly 9000 class candidates tied at 0.1, 100 detections over all nine classes."""
    ref, stages = _oracle("full_capacities")
    net, cfg, img = _device("full_capacities", form)
    assert cfg.rpn_pre_nms_topk == cfg.rpn_post_nms_topk == 1000 and cfg.detections_per_image == 100
    assert stages["n_candidates"] == [9000] and sorted(set(ref[0]["pred_classes"].tolist())) == list(range(9))
    got = net.inference(img.cuda())
    assert net.debug_stage("prop_count", (1,), torch.int32).cpu().tolist() == [1000]
    assert net.debug_stage("det_count", (1,), torch.int32).cpu().tolist() == [100]
    _check_selection(net, cfg, img, stages)
    _check_proposals(net, cfg, img, ref, stages, form, exact=True)
    _check_exact_detections(net, cfg, got, ref, img)


def test_saturated_scores_of_the_real_heads_at_the_deployed_sizes():
    """Case 11.  cls_scale = 60 at 1000 / 1000 / 100: 1000 proposals, 100 detections, with the shared matcher."""
    ref, stages = _oracle("full_saturated_real_heads")
    net, cfg, img = _device("full_saturated_real_heads", "default")
    got = net.inference(img.cuda())
    assert len(ref[0]["proposals"]) == 1000 and len(ref[0]["scores"]) == 100
    assert net.debug_stage("prop_count", (1,), torch.int32).cpu().tolist() == [1000]
    _check_by_matcher(got, ref, need_saturated=True)
