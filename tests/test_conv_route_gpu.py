"""The conv route (csrc/conv_route.hip): one function chooses every conv's kernel, for the launcher and for the planners' op
tables.  ``profile()`` / ``probe_front()`` run the ops one at a time and fail when the family a launch recorded differs from the
op's table entry, so a profile that succeeds says that every name in the table is the kernel that ran."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu


def _last_kernel():
    from peanut_amd import _lib
    return _lib.load().peanut_last_conv_kernel().decode()


def _pred_model(precision="fp32"):
    from peanut_amd.prediction import PEANUT_Prediction_Model
    from peanut_amd.weights import PredCfg, make_seeded_state_dict
    cfg = PredCfg()
    return cfg, PEANUT_Prediction_Model(SimpleNamespace(sem_gpu_id=0), state_dict=make_seeded_state_dict(cfg, seed=0), cfg=cfg,
                                        precision=precision)


def test_one_small_map_names_what_ran():
    """B = 1, 240 x 240, fp32: the skinny kernel, the narrow tiles and the deferred split-K (the stem's 120 output tiles stay
    under the patch kernel's gate: implicit GEMM).  The pyramid's grouped GEMMs are named gemm_skinny by the route alone (no
    planner patches the name in)."""
    from bench import synth_maps
    cfg, m = _pred_model()
    x = synth_maps(1, cfg.in_channels, 240, "cpu", seed0=5).cuda()
    y = m.get_prediction_batch(x, apply_sigmoid=False).clone()
    rows = m.model.profile(x)                       # raises if any conv op's recorded family is not its table entry
    fam = {n: k for n, k, *_ in rows}
    kernels = set(fam.values())
    pyramid = [k for n, k in fam.items() if "psp_modules" in n or "bottleneck.conv[ppm" in n]
    assert pyramid and all(k == "gemm_skinny" for k in pyramid), pyramid
    assert "conv_pw_glds_128x64" in kernels, kernels
    assert any(k.startswith("conv_igemm_") for k in kernels), kernels
    assert "none" not in kernels and "" not in kernels
    assert torch.equal(m.get_prediction_batch(x, apply_sigmoid=False), y)


@pytest.mark.parametrize("batch,precision,families", [
    (2, "fp32", ("conv_pw_glds_", "conv_igemm_")),
    (2, "bf16x6", ("gemm_rs6_",)),
    (10, "fp32", ("conv_pw_ares_128x128", "conv_pw_glds_256x128p", "conv_patch_")),
])
def test_480_maps_name_what_ran_and_profile_changes_nothing(batch, precision, families):
    """480 x 480 maps: profile() succeeds and outputs are bit-equal before and after it on the same handle.  B = 2 in fp32 and
    bf16x6 (gemm_rs); two maps stay under the gates of the tuned kernels (patch_mintiles = 1024, pw_ares_minunits = pw256p_mintiles =
    512 against at most 450 tiles), so B = 10 -- the batch at which tests/test_pred_gpu.py reaches them -- runs the same check on the
    patch, A-resident and persistent 256 x 128 kernels."""
    from bench import synth_maps
    cfg, m = _pred_model(precision)
    x = synth_maps(batch, cfg.in_channels, 480, "cpu", seed0=11).cuda()
    before = m.get_prediction_batch(x, apply_sigmoid=False).clone()
    kernels = {k for _, k, *_ in m.model.profile(x)}
    print(batch, precision, sorted(kernels))
    for want in families:
        assert any(k.startswith(want) for k in kernels), (want, sorted(kernels))
    assert torch.equal(m.get_prediction_batch(x, apply_sigmoid=False), before)


def test_detector_front_end_names_what_ran():
    """The detector at the smallest shape of its tests: the probe succeeds, i.e. every conv op's plan entry (the route, asked when
    the plan is built; Winograd ops as "wino+" + the family of the position GEMM) is the family its launch recorded.  Pointwise
    layers report the conv_pw_* kernels they run on, none packed with 32-channel k-tiles reports conv_igemm_*."""
    from rcnn_cases import small_inputs
    from peanut_amd.rcnn import MaskRCNN
    cfg, sd, img = small_inputs()
    net = MaskRCNN(cfg, sd)
    rows = net.probe_front(img.cuda(), reps=1)
    fams = [k for _, k, _, _ in rows]
    assert any(k.startswith("conv_pw_") for k in fams), fams
    pointwise = 0
    for name, k, _, _ in rows:
        w = sd.get(name + ".weight")
        if w is not None and tuple(w.shape[2:]) == (1, 1) and w.shape[1] % 32 == 0:
            pointwise += 1
            assert not k.startswith("conv_igemm_"), (name, k)
    assert pointwise >= 10, pointwise


def test_route_declines_the_persistent_256x256_kernel_when_the_plan_table_is_too_short():
    """A layer that passes the persistent 256 x 256 kernel's gate by option but gives every workgroup more whole tiles than the
    kernel's plan table holds (kMaxItems = 120: n_full / G + 4 > 120, i.e. 117 tiles per workgroup): the route falls through to
    the next kernel of the cascade -- the one the same layer takes with the gate closed -- and the results are equal bit for bit.
    FusedConv always brings the full split-K scratch, so the decline for a short scratch cannot be made here; it is covered on the
    host by tests/test_persistent_plan_cpu.py.  The smallest layer that crosses the bound: K = 64, N = 256 (one 256-wide n-tile),
    M = 117 x G x 256 rows; one tile per workgroup fewer (116 x G) still runs the persistent kernel."""
    from peanut_amd.ops import FusedConv
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    G = cus - cus % 8
    opts = {"pw256wp_mink": 64, "pw256wp_mintiles": 1, "pw_ares": 0, "pw_bn64_maxk": 0}      # WP_OPTS of test_conv_gpu.py, packed 128 wide
    g = torch.Generator().manual_seed(3)
    w = torch.randn((256, 64, 1, 1), generator=g) * (2.0 / 64) ** 0.5
    shift = torch.randn((256,), generator=g) * 0.1
    on, off = FusedConv(w, None, shift, relu=True, options=opts), FusedConv(w, None, shift, relu=True, options={**opts, "pw256wp_mink": 0})
    x = torch.randn((117 * G, 16, 16, 64), device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))
    under = on(x[:116 * G])
    assert _last_kernel() == "conv_pw_glds_256x256p"
    del under
    y_on = on(x)
    fam_on = _last_kernel()
    y_off = off(x)
    fam_off = _last_kernel()
    assert fam_on != "conv_pw_glds_256x256p" and fam_on == fam_off, (fam_on, fam_off)
    assert torch.equal(y_on, y_off)


def test_route_declines_the_persistent_256x128_kernel_when_the_plan_table_is_too_short():
    """The same fall-through for the persistent 256 x 128 kernel (its gate opened by P256P_OPTS of test_conv_gpu.py): K = 256,
    N = 256 (two 128-wide n-tiles), M = 117 x G x 128 rows = 117 tiles per workgroup -- 3.9 GB of input and of output at G = 256,
    inside the kernel's 4 GiB bound on either tensor -- takes the kernel the layer takes with the gate closed, bit for bit; 116 tiles
    per workgroup still run the persistent kernel."""
    from peanut_amd.ops import FusedConv
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    G = cus - cus % 8
    opts = {"pw256p_mink": 256, "pw256p_mintiles": 8, "pw_ares": 0, "pw256w_mink": 0, "pw256wp_mink": 0, "bn64_maxk": 128}
    g = torch.Generator().manual_seed(5)
    w = torch.randn((256, 256, 1, 1), generator=g) * (2.0 / 256) ** 0.5
    shift = torch.randn((256,), generator=g) * 0.1
    on, off = FusedConv(w, None, shift, relu=True, options=opts), FusedConv(w, None, shift, relu=True, options={**opts, "pw256p_mink": 0})
    x = torch.randn((117 * G // 2, 16, 16, 256), device="cuda", generator=torch.Generator(device="cuda").manual_seed(6))
    under = on(x[:116 * G // 2])
    assert _last_kernel() == "conv_pw_glds_256x128p"
    del under
    y_on = on(x)
    fam_on = _last_kernel()
    y_off = off(x)
    fam_off = _last_kernel()
    assert fam_on != "conv_pw_glds_256x128p" and fam_on == fam_off, (fam_on, fam_off)
    assert torch.equal(y_on, y_off)
