"""Crafted detector inputs for the selection tests (test infrastructure, torch only -- importable without a GPU).

The selection kernels of csrc/rcnn_post.hip (per-level top-k, key sorts, NMS, ordered compactions, the proposal / candidate /
detection capacities) decide on scores.  ``make_seeded_rcnn_state_dict`` keeps those scores distinct on purpose; the cases
here overwrite a few head tensors of such a state dict so that the scores reaching the selection are EXACT (``0 * x + bias =
bias`` bit for bit on the device and in the oracle, every activation being finite), identical on both sides, and adversarial:
runs of equal logits that the top-k cuts through, equal scores across pyramid levels, softmax scores of exactly 1.0f, full
capacities, no valid proposal at all.  tests/test_rcnn_selection_gpu.py runs them through ``peanut_rcnn_inference`` against
oracle/rcnn_ref.py; tests/test_oracles_cpu.py checks, from the oracle alone, that each case has the property it is named for."""
from collections import OrderedDict

import torch

from peanut_amd.rcnn_weights import RcnnCfg, make_seeded_rcnn_state_dict

_OBJ = "proposal_generator.rpn_head.objectness_logits"
_DELTA = "proposal_generator.rpn_head.anchor_deltas"
_CLS = "roi_heads.box_predictor.cls_score"
_BBOX = "roi_heads.box_predictor.bbox_pred"
_MASK = "roi_heads.mask_head.predictor"


def small_cfg(**kw):
    """The suite's small detector: R-50, 96x128 frames -> 128x171, 60 / 40 proposals per level / image, 10 detections."""
    base = dict(depth=50, min_size=128, max_size=256, rpn_pre_nms_topk=60, rpn_post_nms_topk=40, detections_per_image=10)
    base.update(kw)
    return RcnnCfg(**base)


def craft(sd, obj_bias=None, delta_bias=None, cls_bias=None, zero_bbox=False, mask_bias=None, cls_scale=None):
    """A copy of ``sd`` with head tensors overwritten:
    obj_bias [A]        objectness weight = 0, bias = the list: every logit of anchor a equals obj_bias[a] on all levels
    delta_bias [A][4]   anchor-delta weight = 0, bias = the rows (channel a * 4 + (dx, dy, dw, dh))
    cls_bias [K+1]      class-score weight = 0, bias = the list: every proposal has the same score vector
    zero_bbox           box-regression weight and bias = 0: class boxes = proposals
    mask_bias c         mask-predictor weight = 0, bias = c: a constant mask probability
    cls_scale f         class-score weight *= f: the real head's values, saturated"""
    out = OrderedDict((k, v.clone()) for k, v in sd.items())

    def bias_only(name, values):
        out[f"{name}.weight"] = torch.zeros_like(out[f"{name}.weight"])
        b = torch.as_tensor(values, dtype=torch.float32).reshape(-1)
        assert b.shape == out[f"{name}.bias"].shape, (name, b.shape)
        out[f"{name}.bias"] = b.clone()

    if obj_bias is not None:
        bias_only(_OBJ, obj_bias)
    if delta_bias is not None:
        bias_only(_DELTA, delta_bias)
    if cls_bias is not None:
        bias_only(_CLS, cls_bias)
    if zero_bbox:
        bias_only(_BBOX, torch.zeros_like(out[f"{_BBOX}.bias"]))
    if mask_bias is not None:
        bias_only(_MASK, torch.full_like(out[f"{_MASK}.bias"], float(mask_bias)))
    if cls_scale is not None:
        out[f"{_CLS}.weight"] = out[f"{_CLS}.weight"] * float(cls_scale)
    return out


_Z = [[0.0, 0.0, 0.0, 0.0]] * 3
_TIED_OBJ = [0.5, 2.0, -1.0]
_SAT_CLS = [0.0, 0.0, 0.0, 40.0] + [0.0] * 6          # +40 on class 3: softmax = exactly 1.0f there, e^-40 elsewhere

# name -> (size, knobs).  size "small": small_cfg(), seed 7, two 96x128 frames (the frames of test_rcnn_gpu.py's small_net);
# "full": the deployed selection sizes (1000 / 1000 / 100) on an R-50 body, one 480x640 frame.
CASES = {
    "rpn_ties": ("small", dict(obj_bias=_TIED_OBJ)),
    "rpn_ties_anchors": ("small", dict(obj_bias=_TIED_OBJ, delta_bias=_Z)),
    "all_tied": ("small", dict(obj_bias=[1.0, 1.0, 1.0], delta_bias=_Z, cls_bias=[0.0] * 10, zero_bbox=True, mask_bias=1.0)),
    "saturated": ("small", dict(cls_bias=_SAT_CLS, zero_bbox=True)),
    "saturated_real_heads": ("small", dict(cls_scale=60.0)),
    "select_then_filter": ("small", dict(obj_bias=_TIED_OBJ, delta_bias=[[0.0] * 4, [float("inf"), 0.0, 0.0, 0.0], [0.0] * 4])),
    "no_proposal": ("small", dict(delta_bias=[[1e4, 1e4, 0.0, 0.0]] * 3)),
    "clamp": ("small", dict(delta_bias=[[0.0, 0.0, 10.0, 10.0]] * 3)),
    "nan_objectness": ("small", dict(obj_bias=[0.5, float("nan"), -1.0])),
    "full_capacities": ("full", dict(obj_bias=_TIED_OBJ, delta_bias=_Z, cls_bias=[0.0] * 10, zero_bbox=True, mask_bias=1.0)),
    "full_saturated_real_heads": ("full", dict(cls_scale=60.0)),
}


def small_inputs():
    """-> (cfg, seeded state dict, two 96x128 uint8 frames): the small detector every stage test runs (test_rcnn_gpu.py's small_net)."""
    cfg = small_cfg()
    sd = make_seeded_rcnn_state_dict(cfg, seed=7)
    img = torch.randint(0, 256, (2, 96, 128, 3), generator=torch.Generator().manual_seed(11), dtype=torch.uint8)
    return cfg, sd, img


def make_case(name):
    """-> (cfg, crafted state dict, uint8 frames [B,H,W,3] on the CPU)."""
    size, knobs = CASES[name]
    if size == "small":
        cfg, sd, img = small_inputs()
    else:
        cfg = RcnnCfg(depth=50)
        sd = make_seeded_rcnn_state_dict(cfg, seed=3)
        img = torch.randint(0, 256, (1, 480, 640, 3), generator=torch.Generator().manual_seed(5), dtype=torch.uint8)
    if "nan_objectness" == name:      # torch.tensor(float('nan')): the quiet NaN with the sign bit clear (it must rank FIRST)
        assert int(torch.tensor(float("nan")).view(torch.int32)) == 0x7FC00000
    return cfg, craft(sd, **knobs), img


def oracle_run(name):
    """The oracle's instances and stage outputs of a case, with torch capped at 16 threads (the restatement is thousands of
    small ops: a larger pool only adds latency)."""
    from oracle import rcnn_ref
    cfg, sd, img = make_case(name)
    threads = torch.get_num_threads()
    torch.set_num_threads(min(threads, 16))
    try:
        stages = {}
        with torch.no_grad():
            ref = rcnn_ref.inference(sd, img, cfg, vectorised=True, stages=stages)
    finally:
        torch.set_num_threads(threads)
    return ref, stages


def level_ks(cfg, h, w):
    """[(offset, k, n)] of the five pyramid levels of an h x w frame: where a level's selection starts inside the stage buffers
    ``sel_idx`` / ``sel_score``, how many anchors it selects and how many it has."""
    from peanut_amd.rcnn_weights import padded_hw, resized_hw
    ph, pw = padded_hw(*resized_hw(h, w, cfg), cfg)
    out, off = [], 0
    for l in range(5):
        s = min(4 << l, 32)
        lh, lw = -(-ph // s), -(-pw // s)
        if l == 4:                      # p6: max_pool2d(kernel 1, stride 2) of p5
            lh, lw = (lh - 1) // 2 + 1, (lw - 1) // 2 + 1
        n = lh * lw * cfg.num_anchors
        k = min(n, cfg.rpn_pre_nms_topk)
        out.append((off, k, n))
        off += k
    return out


def match_detections(gi, ri):
    """One image: every detection of the oracle (``ri``) matched one to one by a detection of the device (``gi``) of the same
    class with score within 1e-4 and box within 0.05 px -- the nearest rank among the candidates -- and a rank may differ only
    inside a run of scores closer than 2e-4.  -> (perm [n]: rank in gi of the oracle's i-th, number of moved ranks,
    max |score diff|, max |box diff|, mask IoU over the image)."""
    n = len(ri["scores"])
    assert len(gi["scores"]) == n > 0
    gs, gb, gc = gi["scores"].cpu(), gi["pred_boxes"].cpu(), gi["pred_classes"].cpu()
    rs, rb, rc = ri["scores"], ri["pred_boxes"], ri["pred_classes"]
    ok = (gc[None, :] == rc[:, None]) & ((gs[None, :] - rs[:, None]).abs() <= 1e-4) & \
         ((gb[None, :, :] - rb[:, None, :]).abs().amax(2) <= 5e-2)                      # [ref i, got j]
    perm = torch.full((n,), -1, dtype=torch.int64)
    taken = torch.zeros(n, dtype=torch.bool)
    for i in range(n):
        cand = torch.nonzero(ok[i] & ~taken).flatten()
        assert len(cand) > 0, f"oracle detection {i} (class {int(rc[i])}, score {float(rs[i]):.6f}) has no counterpart"
        j = int(cand[(cand - i).abs().argmin()])
        perm[i] = j
        taken[j] = True
    moved = torch.nonzero(perm != torch.arange(n)).flatten()
    for i in moved.tolist():     # a rank can only differ inside a run of near-equal scores
        lo, hi = min(i, int(perm[i])), max(i, int(perm[i]))
        assert float(rs[lo] - rs[hi]) <= 2e-4
    worst_score = (gs[perm] - rs).abs().max().item()
    worst_box = (gb[perm] - rb).abs().max().item()
    gm, rm = gi["pred_masks"].cpu()[perm], ri["pred_masks"]
    inter, union = (gm & rm).sum().item(), (gm | rm).sum().item()
    return perm, len(moved), worst_score, worst_box, inter / max(union, 1)
