"""The cases of tests/small_map_cases.py, checked without a GPU: they are in the regime they were chosen for, and the reference
they are compared with is good enough to hold a kernel to."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import small_map_cases as sm      # noqa: E402


def test_case_list_is_the_agreed_one():
    assert len(sm.SMALL_MAPS) == 11 and len(set(sm.SMALL_MAPS)) == 11 and set(sm.LAYER4) == set(sm.SMALL_MAPS)
    assert sm.CORE == sm.SMALL_MAPS[:5] and sm.CORE[0] == (1, 16, 16) and (9, 16, 16) in sm.CORE and (1, 16, 720) in sm.CORE
    assert all(min(h, w) >= sm.MIN_SIDE for _, h, w in sm.SMALL_MAPS)


@pytest.mark.parametrize("shape", sm.SMALL_MAPS, ids=sm.shape_id)
def test_feature_map_sizes(shape):
    """layer4 of every case has the size its comment promises: a change of the list cannot silently leave the regime (pyramid
    scale 6 at or above the map on one axis at least, dilation 4 above it)."""
    cfg = sm.cfg_for(False)
    t = sm.ref_taps(cfg, shape)
    assert tuple(t["layer4"].shape) == (shape[0], 2048) + sm.LAYER4[shape]
    assert min(sm.LAYER4[shape]) <= max(cfg.pool_scales)
    assert t["ppm_table"].shape[2] == sum(k * k for k in cfg.pool_scales)


@pytest.mark.parametrize("align_corners", [False, True], ids=["ac0", "ac1"])
def test_fp32_oracle_is_within_a_quarter_of_the_tolerance_of_fp64(align_corners):
    """The oracle run in float32 -- what every other forward test compares with -- against the same oracle in float64, on every
    case: within TOL / 4 on the logits and on the sigmoid outputs (measured: 4.2e-6 for align_corners = False, 1.14e-5 for True,
    worst at 16 x 720), so the reference alone uses under a quarter of what the kernels are held to."""
    cfg = sm.cfg_for(align_corners)
    worst = (0.0, None)
    for shape in sm.SMALL_MAPS:
        r64, r32 = sm.ref_logits(cfg, shape), sm.ref_logits(cfg, shape, torch.float32)
        assert r64.dtype == torch.float64 and r32.dtype == torch.float32
        assert tuple(r64.shape) == (shape[0], cfg.num_classes, shape[1], shape[2])
        err = (r32.double() - r64).abs().max().item()
        errp = (torch.sigmoid(r32).double() - torch.sigmoid(r64)).abs().max().item()
        worst = max(worst, (err, shape))
        assert err <= sm.TOL / 4 and errp <= sm.TOL / 4, f"{shape}: logits {err:.3e} sigmoid {errp:.3e}"
    print(f"align_corners={align_corners}: fp32 oracle vs fp64 oracle, worst max-abs {worst[0]:.3e} at {worst[1]} (TOL / 4 = {sm.TOL / 4:.2e})")


def test_size_boundary_constants():
    """16 is accepted, 15 is not (csrc/pred_api.hip: get_plan); the GPU file uses these constants.  The reference itself serves
    15 x 16, so the bound is the library's, not the model's."""
    assert (sm.MIN_SIDE, sm.BELOW_MIN) == (16, 15)
    assert min(min(h, w) for _, h, w in sm.SMALL_MAPS) == sm.MIN_SIDE
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "peanut_amd", "csrc", "pred_api.hip")).read()
    assert f"H < {sm.MIN_SIDE} || W < {sm.MIN_SIDE}" in src
    from oracle import pspnet_ref
    cfg = sm.cfg_for(False)
    y = pspnet_ref.forward_batch(sm.state_dict(cfg), sm.inputs((1, sm.BELOW_MIN, sm.MIN_SIDE)), cfg)
    assert tuple(y.shape) == (1, cfg.num_classes, sm.BELOW_MIN, sm.MIN_SIDE) and bool(torch.isfinite(y).all())
