"""Sliding-window and flip-averaged inference (ABI 24; ``peanut_pred_inference``, ``HipSegmentor.inference``) on the device.

1. Against the reference's own ``slide_inference`` / ``inference`` / ``aug_test`` (tests/golden/infer_golden.npz) at the suite's
   tolerance, every case and aug list of tests/infer_cases.py.
2. Bit for bit against the stated rule applied in torch to ONE plain forward of the staged batch, rebuilt here in the contracted
   order: this pins the gather, the window order, the IEEE division and the un-flip independently of the forward's rounding.
3. The degenerate forms, 4. the callers, 5. misuse, 6. stale memory.
Every comparison prints the figure it asserts on."""
import ctypes as C
import dataclasses
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import infer_cases as ic                                      # noqa: E402
from workspace_cases import first_difference, poisoned, same  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = ic.TOL
EINVAL = -2


def _cfg(case=None, flips=(0,)):
    """The PredCfg a config file with the case's test_cfg and these flips parses to (case None: test_cfg whole)."""
    from peanut_amd.weights import PredCfg
    augs = tuple((bool(f), ic.FLIP_NAMES.get(f, "horizontal")) for f in flips)
    if case is None:
        return PredCfg(augs=augs)
    c = ic.CASES[case]
    return PredCfg(test_mode="slide", crop_size=c["crop"], stride=c["stride"], augs=augs)


def _model(cfg=None, **kw):
    from peanut_amd.prediction import PEANUT_Prediction_Model
    from peanut_amd.weights import PredCfg, make_seeded_state_dict
    cfg = cfg or PredCfg()
    return PEANUT_Prediction_Model(SimpleNamespace(sem_gpu_id=0), state_dict=make_seeded_state_dict(PredCfg(), 0), cfg=cfg, **kw)


def _infer(seg, x, case, flips, **kw):
    """``seg.inference`` under the case's test_cfg and these flips: the handle is the same for every cfg, only the descriptor differs."""
    old = seg.cfg
    seg.cfg = dataclasses.replace(old, **{k: getattr(_cfg(case, flips), k) for k in ("test_mode", "crop_size", "stride", "augs")})
    try:
        return seg.inference(x, **kw)
    finally:
        seg.cfg = old


@pytest.fixture(scope="module")
def plain():
    """The default model: fp32, the stock cfg.  Its handle serves every descriptor of this file."""
    m = _model()
    yield m
    del m


@pytest.fixture(scope="module")
def golden():
    return np.load(ic.GOLDEN)


_XD = {}


def _xd(case):
    if case not in _XD:
        _XD[case] = ic.inputs(case).cuda()
    return _XD[case]


def _wins(case):
    c = ic.CASES[case]
    return ic.windows(c["H"], c["W"], c["crop"], c["stride"])[0]


# ---- 1. the reference ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("augs", list(ic.AUG_LISTS))
@pytest.mark.parametrize("case", list(ic.CASES))
def test_matches_the_reference(plain, golden, case, augs):
    ref = torch.from_numpy(golden[ic.key(case, augs)])
    got = _infer(plain.model, _xd(case), case, ic.AUG_LISTS[augs]).cpu()
    got_p = _infer(plain.model, _xd(case), case, ic.AUG_LISTS[augs], apply_sigmoid=True).cpu()
    err, errp = (got - ref).abs().max().item(), (got_p - torch.sigmoid(ref)).abs().max().item()
    print(f"{case}/{augs}: logits {err:.3e} sigmoid {errp:.3e} (bound {TOL})")
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    assert err <= TOL and errp <= TOL


@pytest.mark.parametrize("precision, bound", [("bf16x6", 5e-5), ("fp16x3", 5e-5), ("bf16x3", 5e-4)])
def test_emulated_precisions_match_the_reference(golden, precision, bound):
    """Case A with [none, horizontal]; the bounds of tests/test_small_maps_gpu.py."""
    m = _model(_cfg("A", (0, 1)), precision=precision)
    ref = torch.from_numpy(golden[ic.key("A", "none_h")])
    got = m.get_prediction_batch(_xd("A"), apply_sigmoid=False).cpu()
    got_p = m.get_prediction_batch(_xd("A")).cpu()
    err, errp = (got - ref).abs().max().item(), (got_p - torch.sigmoid(ref)).abs().max().item()
    print(f"A/none_h {precision}: logits {err:.3e} sigmoid {errp:.3e} (bound {bound})")
    assert err <= bound and errp <= bound


# ---- 2. bit for bit ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_batch", [0, 4])
@pytest.mark.parametrize("case", list(ic.CASES))
def test_equals_the_stated_rule_bit_for_bit(plain, case, max_batch):
    c = ic.CASES[case]
    x, wins = _xd(case), _wins(case)
    for name, flips in ic.AUG_LISTS.items():
        staged = ic.staged_batch(x, wins, flips).contiguous()
        chunk = max_batch or staged.shape[0]
        logits = torch.cat([plain.get_prediction_batch(staged[i:i + chunk].contiguous(), apply_sigmoid=False)
                            for i in range(0, staged.shape[0], chunk)])
        want = ic.combine(logits, wins, flips, c["B"], c["H"], c["W"])
        got = _infer(plain.model, x, case, flips, max_batch=max_batch)
        assert same(got, want), f"{case}/{name} max_batch {max_batch}: {first_difference(got, want)}"
    print(f"{case}: {len(wins)} windows of {wins[0][2] - wins[0][0]} x {wins[0][3] - wins[0][1]}, max_batch {max_batch}: all aug lists bit-identical")


def test_whole_mode_with_flips_equals_the_stated_rule_bit_for_bit(plain):
    """test_cfg whole with the flipped images of the pipeline: one window, no division by a count."""
    for case in ("A", "B"):
        c = ic.CASES[case]
        x, wins = _xd(case), [(0, 0, c["H"], c["W"])]
        for flips in ((0, 1), (0, 0, 1, 2), (2,), (1,)):
            logits = plain.get_prediction_batch(ic.staged_batch(x, wins, flips).contiguous(), apply_sigmoid=False)
            want = ic.combine(logits, wins, flips, c["B"], c["H"], c["W"], slide=False)
            got = _infer(plain.model, x, None, flips)
            assert same(got, want), f"{case} whole {flips}: {first_difference(got, want)}"


@pytest.mark.parametrize("case", list(ic.CASES))
def test_the_two_glue_launches_alone_bit_for_bit(case):
    """``peanut_pred_infer_gather`` against the staged batch rebuilt in torch, ``peanut_pred_infer_combine`` on random logits (signed
    zeros among them) against the rule in torch -- with three images as well, where a reciprocal multiply would differ from the
    division by 3; on a 16-byte aligned and on a misaligned view (the scalar path of case B)."""
    from peanut_amd import prediction as P
    c = ic.CASES[case]
    B, H, Wd = c["B"], c["H"], c["W"]
    x, wins = _xd(case), _wins(case)
    g = torch.Generator().manual_seed(17)
    for flips in list(ic.AUG_LISTS.values()) + [(1, 2, 0)]:
        d = P.infer_descriptor("slide", c["crop"], c["stride"], flips)
        staged = P.infer_gather(x, d)
        assert same(staged, ic.staged_batch(x, wins, flips).contiguous()), (case, flips)
        logits = torch.randn((staged.shape[0], 6, staged.shape[2], staged.shape[3]), generator=g)
        logits[:, :, ::3, ::5] = -0.0
        logits = logits.cuda()
        for sig in (False, True):
            want = ic.combine(logits, wins, flips, B, H, Wd)
            got = P.infer_combine(logits, d, B, H, Wd, apply_sigmoid=sig)
            if sig:
                assert (got - torch.sigmoid(want)).abs().max().item() <= 5e-7      # (expf and one division on values in [0, 1])
            else:
                assert same(got, want), f"{case} {flips}: {first_difference(got, want)}"
        # the same through buffers that start 4 bytes off a 16-byte boundary
        xo = torch.empty((x.numel() + 1,), device="cuda")[1:].view_as(x).copy_(x)
        lo = torch.empty((logits.numel() + 1,), device="cuda")[1:].view_as(logits).copy_(logits)
        assert xo.data_ptr() % 16 == 4 and same(P.infer_gather(xo, d), staged)
        assert same(P.infer_combine(lo, d, B, H, Wd), ic.combine(logits, wins, flips, B, H, Wd))
    dw = P.infer_descriptor("whole", flips=(0, 1, 2))
    whole = [(0, 0, H, Wd)]
    assert same(P.infer_gather(x, dw), ic.staged_batch(x, whole, (0, 1, 2)).contiguous())
    lw = torch.randn((3 * B, 6, H, Wd), generator=g).cuda()
    assert same(P.infer_combine(lw, dw, B, H, Wd), ic.combine(lw, whole, (0, 1, 2), B, H, Wd, slide=False))
    with pytest.raises(ValueError):
        P.infer_combine(lw[:-1], dw, B, H, Wd)


# ---- 3. degenerate forms -------------------------------------------------------------------------------------------------------
def test_degenerate_forms_equal_the_plain_forward(plain):
    seg = plain.model
    for case in ("A", "B"):                                   # whole + [none] through inference
        x = _xd(case)
        assert same(_infer(seg, x, None, (0,)), seg.forward_logits(x)), case
        assert same(_infer(seg, x, None, (0,), apply_sigmoid=True), seg.forward_logits(x, apply_sigmoid=True)), case
    x = _xd("E")                                              # crop >= image: one window of the image's size
    assert same(_infer(seg, x, "E", (0,)), seg.forward_logits(x))


def test_a_batch_equals_its_samples_within_tol(plain):
    """B = 3 against three B = 1 calls: within TOL only -- the row groups of the pyramid pooling are chosen from the batch size, so
    the last bits of a logit depend on it (include/peanut_hip.h, "Conv arithmetic")."""
    x = _xd("A")
    flips = ic.AUG_LISTS["two_dirs"]
    full = _infer(plain.model, x, "A", flips)
    worst = 0.0
    for b in range(x.shape[0]):
        one = _infer(plain.model, x[b:b + 1].contiguous(), "A", flips)
        worst = max(worst, (one[0] - full[b]).abs().max().item())
    print(f"A/two_dirs: B = 3 against 3 x B = 1: {worst:.3e} (bound {TOL})")
    assert worst <= TOL


# ---- 4. callers ----------------------------------------------------------------------------------------------------------------
def test_callers_honour_a_slide_and_flip_config(golden, monkeypatch):
    from peanut_amd import prediction as P
    calls = []
    real = P.HipSegmentor.inference
    monkeypatch.setattr(P.HipSegmentor, "inference", lambda self, *a, **k: (calls.append(1), real(self, *a, **k))[1])
    m = _model(_cfg("B", (0, 1)))
    ref = golden[ic.key("B", "none_h")]
    full_map = ic.inputs("B")[0].numpy()
    prob = m.get_prediction(full_map)
    logits = P.run_inference(m.model, full_map)
    batch = m.get_prediction_batch(_xd("B")).cpu().numpy()
    ref_p = torch.sigmoid(torch.from_numpy(ref)).numpy()
    errs = (np.abs(prob - ref_p[0]).max(), np.abs(logits[0] - ref[0]).max(), np.abs(batch - ref_p).max())
    print(f"B/none_h through get_prediction {errs[0]:.3e}, run_inference {errs[1]:.3e}, get_prediction_batch {errs[2]:.3e} (bound {TOL})")
    assert prob.shape == ref.shape[1:] and prob.dtype == np.float32 and len(logits) == 1 and logits[0].shape == ref.shape[1:]
    assert max(errs) <= TOL
    assert len(calls) == 3
    # precision="auto": the range-checked path goes through inference as well
    auto = _model(_cfg("B", (0, 1)), precision="auto")
    got = auto.get_prediction_batch(_xd("B"), apply_sigmoid=False).cpu().numpy()
    print(f"B/none_h precision auto: {np.abs(got - ref).max():.3e}")
    assert np.abs(got - ref).max() <= TOL and len(calls) == 4


def test_the_default_config_never_enters_inference(plain, monkeypatch):
    from peanut_amd import prediction as P
    calls = []
    monkeypatch.setattr(P.HipSegmentor, "inference", lambda self, *a, **k: calls.append(1))
    x = _xd("B")
    want = plain.model.forward_logits(x, apply_sigmoid=True)
    assert plain.model.cfg.plain_inference
    assert same(plain.get_prediction_batch(x), want)
    assert np.array_equal(plain.get_prediction(ic.inputs("B")[0].numpy()), want[0].cpu().numpy())
    assert np.array_equal(P.run_inference(plain.model, ic.inputs("B")[0].numpy())[0], plain.model.forward_logits(x)[0].cpu().numpy())
    assert calls == []


# ---- 5. misuse -----------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing(plain):
    from peanut_amd import _lib
    from peanut_amd import prediction as P
    seg = plain.model
    lib = seg._lib
    c = ic.CASES["A"]
    B, H, Wd = c["B"], c["H"], c["W"]
    x = _xd("A")
    out = torch.full((B, 6, H, Wd), 12345.0, device="cuda")
    torch.cuda.synchronize()

    def slide(crop=c["crop"], stride=c["stride"], flips=(0, 1), **kw):
        return P.infer_descriptor("slide", crop, stride, flips, **kw)

    def call(d, xp=None, op=None, b=B, h=H, w=Wd):
        return lib.peanut_pred_inference(seg._h, C.byref(d) if d is not None else None, x.data_ptr() if xp is None else xp,
                                         out.data_ptr() if op is None else op, b, h, w, 0)
    bad = {}
    for n in (0, 5):
        d = slide(); d.n_augs = n; bad[f"n_augs {n}"] = d
    d = slide(); d.flip[1] = 3; bad["flip code 3"] = d
    bad["max_batch -1"] = slide(max_batch=-1)
    bad["uncovered rows"] = slide(crop=(16, 32), stride=(20, 20))
    bad["33 windows on an axis"] = slide(crop=(16, 16), stride=(16, 1))
    bad["window of 15"] = slide(crop=(15, 32), stride=(8, 20))
    d = slide(); d.mode = 7; bad["mode 7"] = d
    for what, d in bad.items():
        assert call(d) == EINVAL, what
        assert lib.peanut_last_error()
    assert call(slide(), b=0) == EINVAL
    assert call(None) == EINVAL
    assert lib.peanut_pred_inference(None, C.byref(slide()), x.data_ptr(), out.data_ptr(), B, H, Wd, 0) == EINVAL
    assert lib.peanut_pred_inference(seg._h, C.byref(slide()), None, out.data_ptr(), B, H, Wd, 0) == EINVAL
    assert lib.peanut_pred_inference(seg._h, C.byref(slide()), x.data_ptr(), None, B, H, Wd, 0) == EINVAL
    # out_dev inside in_dev, and in_dev's last plane inside out_dev
    big = torch.zeros((B * 14 * H * Wd + B * 6 * H * Wd,), device="cuda")
    torch.cuda.synchronize()
    assert call(slide(), xp=big.data_ptr(), op=big.data_ptr() + 4 * H * Wd) == EINVAL
    assert "overlaps" in lib.peanut_last_error().decode()
    assert call(slide(), xp=big.data_ptr() + 4 * (B * 6 * H * Wd - 1), op=big.data_ptr()) == EINVAL
    torch.cuda.synchronize()
    assert bool((out == 12345.0).all()) and float(big.abs().max()) == 0.0
    # the Python surface refuses what it can see
    with pytest.raises(ValueError):
        seg.inference(x[:, :3].contiguous())
    with pytest.raises(ValueError):
        seg.inference(x, out=torch.empty((1, 6, H, Wd), device="cuda"))
    with pytest.raises(_lib.PeanutHipError, match="at least 16"):
        _infer(seg, torch.zeros((1, 14, 15, 40), device="cuda"), None, (0,))
    # and adjacent buffers are not an overlap
    assert call(slide(), xp=big.data_ptr(), op=big.data_ptr() + 4 * B * 14 * H * Wd) == 0
    torch.cuda.synchronize()


def test_workspace_bytes_cover_the_staging(plain):
    seg = plain.model
    c = ic.CASES["A"]
    old = seg.cfg
    seg.cfg = _cfg("A", (0, 1))
    try:
        n = 2 * c["B"] * 9
        staging = n * (14 + 6) * 24 * 32 * 4
        assert seg.inference_workspace_bytes(c["B"], c["H"], c["W"]) == staging + seg.workspace_bytes(n, 24, 32)
        assert seg.inference_workspace_bytes(c["B"], c["H"], c["W"], max_batch=4) == staging + seg.workspace_bytes(4, 24, 32)
    finally:
        seg.cfg = old


# ---- 6. stale memory -----------------------------------------------------------------------------------------------------------
def test_result_does_not_depend_on_what_the_buffers_held(plain):
    """A fresh handle whose every allocation starts as 0xFF bytes (``debug_poison_alloc``: the staging buffers come from
    ``dev_alloc``), before and after a call at a larger shape, against the module's handle."""
    flips = ic.AUG_LISTS["two_dirs"]
    want = _infer(plain.model, _xd("A"), "A", flips).clone()
    torch.cuda.synchronize()
    with poisoned():
        m = _model()
        got = _infer(m.model, _xd("A"), "A", flips).clone()
        g = torch.Generator().manual_seed(5)
        larger = (torch.rand((2, 14, 72, 104), generator=g) > 0.7).float().cuda()
        big = _infer(m.model, larger, "A", (0, 1))            # 2 x 2 x 16 windows: both stagings and the workspace grow
        again = _infer(m.model, _xd("A"), "A", flips).clone()
        torch.cuda.synchronize()
    assert bool(torch.isfinite(big).all())
    assert same(got, want), first_difference(got, want)
    assert same(again, want), first_difference(again, want)
