"""The per-frame glue kernels at their decision boundaries: ``preprocess_obs`` / ``preprocess_obs_batch``
(csrc/preprocess.hip) against ``oracle.agent_ref.preprocess_obs_ref`` and ``accumulate_instances`` (csrc/seg_accum.hip) against
the loop of segmentation.py:47-60, on the cases of tests/frame_glue_cases.py.  tests/test_frame_glue_cpu.py proves without a GPU
that every case holds the boundary it is named after and that each neighbouring rule (``>=`` for ``>``, statistics over the
sampled rows, one folded constant, ``<=`` gates, float64 gates) moves the expectation of a named case, so each test here fails
under the matching mistake in the kernel.

Everything is bit-exact: the outputs are float32 values the reference computes in the same order (contraction is off in
preprocess.hip), copies, or small integers.  No tolerance anywhere.  The fused entry's copy of the gates
(``paste_accumulate_kernel``) is held to ``accumulate_instances`` at the same boundaries by
tests/test_rcnn_gpu.py::test_semantic_entry_equals_inference_plus_accumulation."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import frame_glue_cases as fg

pytestmark = pytest.mark.gpu

PRE = fg.preprocess_cases()
ACC = fg.accumulation_cases()
EINVAL = -2
SENTINEL = -12345.5


def _dev(fr):
    return tuple(torch.from_numpy(v).cuda() for v in (fr.rgb, fr.depth, fr.sem))


def _same_bits(got: torch.Tensor, ref: np.ndarray) -> bool:
    got = got.cpu().numpy()
    return got.shape == ref.shape and got.dtype == ref.dtype == np.float32 and np.array_equal(got.view(np.uint32), ref.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------------
# preprocess
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PRE))
def test_preprocess_obs_matches_the_reference(name):
    from peanut_amd.agent_helper import preprocess_obs
    fr = PRE[name]
    ref = fg.preprocess_ref(fr)
    got = preprocess_obs(*_dev(fr), fr.args)
    c = fr.claims
    assert got.shape == (1, 4 + c["ncat"], c["H"] // c["ds"], c["W"] // c["ds"])
    assert _same_bits(got[0], ref), np.argwhere(got[0].cpu().numpy() != ref)[:8]


@pytest.mark.parametrize("name", ["mean90[0]", "far099[0]", "geometry[130x6/1,ncat=21]"])
def test_preprocess_obs_wrapper_forms(name):
    from peanut_amd.agent_helper import preprocess_obs
    fr = PRE[name]
    ref = fg.preprocess_ref(fr)
    forms = fg.preprocess_forms(fr, "cuda")
    assert not forms["depth_slice"][1].is_contiguous() and not forms["rgb_view"][0].is_contiguous() and not forms["sem_view"][2].is_contiguous()
    for form, (rgb, depth, sem) in forms.items():
        assert _same_bits(preprocess_obs(rgb, depth, sem, fr.args)[0], ref), form


@pytest.mark.parametrize("E", [1, 16])
def test_preprocess_obs_batch_matches_the_reference_frame_by_frame(E):
    from peanut_amd.agent_helper import preprocess_obs, preprocess_obs_batch
    frames = fg.batch_frames(E)
    args = frames[0].args
    rgb, depth, sem = (torch.from_numpy(np.stack([getattr(f, k) for f in frames])).cuda() for k in ("rgb", "depth", "sem"))
    got = preprocess_obs_batch(rgb, depth, sem, args)
    assert got.shape == (E, 14, 10, 12)
    for e, fr in enumerate(frames):
        assert _same_bits(got[e], fg.preprocess_ref(fr)), (e, fr.name)
        assert torch.equal(got[e:e + 1], preprocess_obs(rgb[e], depth[e], sem[e], args)), (e, fr.name)
    assert torch.equal(preprocess_obs_batch(rgb, depth[..., 0], sem, args), got)                 # depth [E,H,W]
    perm = torch.tensor(fg.BATCH_PERM[:E] if E == 16 else [0], device="cuda")
    assert torch.equal(preprocess_obs_batch(rgb[perm], depth[perm], sem[perm], args), got[perm])
    if E == 16:     # the frames as non-contiguous views of a wider batch: every other frame of 32
        wide = [torch.zeros((2 * E,) + tuple(t.shape[1:]), dtype=t.dtype, device="cuda") for t in (rgb, depth, sem)]
        for w, t in zip(wide, (rgb, depth, sem)):
            w[::2] = t
        assert not wide[1][::2].is_contiguous()
        assert torch.equal(preprocess_obs_batch(wide[0][::2], wide[1][::2], wide[2][::2], args), got)


def test_preprocess_refusals_leave_obs_untouched():
    """H % ds, W % ds, ncat = 0, ds = 0, E = 0 and E = 17 return PEANUT_EINVAL before anything is launched.  The buffers would
    hold every one of these geometries, were a launch made."""
    from peanut_amd import _lib
    from peanut_amd.agent_helper import preprocess_obs, preprocess_obs_batch
    lib = _lib.load()
    E, H, W, ncat = 17, 44, 52, 10
    rgb = torch.zeros((E, H, W, 3), dtype=torch.uint8, device="cuda")
    depth = torch.rand((E, H, W), device="cuda")
    sem = torch.rand((E, H, W, ncat), device="cuda")
    obs = torch.full((E * (4 + ncat) * H * W,), SENTINEL, device="cuda")
    stream = _lib.current_stream_ptr(obs.device)
    p = (rgb.data_ptr(), depth.data_ptr(), sem.data_ptr())
    for h, w, nc, ds in ((42, 48, 10, 4), (40, 50, 10, 4), (40, 48, 0, 4), (40, 48, 10, 0), (40, 48, -1, 4)):
        assert lib.peanut_preprocess_obs(*p, h, w, nc, ds, 0.5, 5.0, obs.data_ptr(), stream) == EINVAL, (h, w, nc, ds)
        assert b"peanut_preprocess_obs" in lib.peanut_last_error()
        for e in (1, 16):
            assert lib.peanut_preprocess_obs_batch(*p, e, h, w, nc, ds, 0.5, 5.0, obs.data_ptr(), stream) == EINVAL, (e, h, w, nc, ds)
    for e in (0, 17, -1):
        assert lib.peanut_preprocess_obs_batch(*p, e, 40, 48, 10, 4, 0.5, 5.0, obs.data_ptr(), stream) == EINVAL, e
        assert b"PEANUT_MAP_MAX_BATCH" in lib.peanut_last_error()
    assert lib.peanut_preprocess_obs(*p, 40, 48, 10, 4, 0.5, 5.0, None, stream) == EINVAL
    torch.cuda.synchronize()
    assert bool((obs == SENTINEL).all())
    # the same through the wrappers: an error, never a shortened frame
    fr = fg.mean90()
    r, d, s = _dev(fr)
    with pytest.raises(_lib.PeanutHipError):
        preprocess_obs(r[:38], d[:38], s[:38], fr.args)                                           # H % ds
    with pytest.raises(_lib.PeanutHipError):
        preprocess_obs(r, d, s[:, :, :0], fr.args)                                                # ncat = 0
    with pytest.raises(_lib.PeanutHipError):
        preprocess_obs_batch(r[None].repeat(17, 1, 1, 1), d[None].repeat(17, 1, 1, 1), s[None].repeat(17, 1, 1, 1), fr.args)
    with pytest.raises(_lib.PeanutHipError):
        preprocess_obs_batch(r[None][:0], d[None][:0], s[None][:0], fr.args)                      # E = 0


# ---------------------------------------------------------------------------------------------------------------------------------
# accumulation
# ---------------------------------------------------------------------------------------------------------------------------------
def _accumulate(c, masks=None, classes=None, scores=None):
    from peanut_amd.segmentation import accumulate_instances
    return accumulate_instances((c.masks if masks is None else masks).cuda(), (c.classes if classes is None else classes).cuda(),
                                (c.scores if scores is None else scores).cuda(), c.n_cats, c.thr, c.goal_thr, c.goal_cat).cpu()


@pytest.mark.parametrize("name", list(ACC))
def test_accumulate_instances_matches_the_reference_loop(name):
    c = ACC[name]
    ref = fg.case_ref(c)
    got = _accumulate(c)
    assert got.shape == ref.shape == fg.ACC_HW + (c.n_cats + 1,)
    assert torch.equal(got, ref), (got - ref).abs().sum((0, 1))
    assert float(got[..., c.n_cats].abs().max()) == 0.0
    if name.startswith("counts"):
        y, x = fg.COUNT_PIXEL
        assert got[y, x, 2] == 100.0 and got[y, x, 6] == 50.0


def test_accumulate_instances_wrapper_forms():
    """classes int64 / int32, scores float64 holding the float32 values (the wrapper converts: the gates are float32, as the
    reference's ``pred_instances.scores`` is), masks bool / uint8 as non-contiguous views, n = 0 with a goal category."""
    from peanut_amd.segmentation import accumulate_instances
    c = fg.gates("present", "default")
    ref = fg.case_ref(c)
    assert c.classes.dtype == torch.int64 and c.scores.dtype == torch.float32
    assert torch.equal(_accumulate(c, classes=c.classes.to(torch.int32)), ref)
    assert torch.equal(_accumulate(c, scores=c.scores.double()), ref)
    n, (H, W) = len(c.classes), fg.ACC_HW
    for dtype in (torch.bool, torch.uint8):
        wide = torch.ones((n, H, 2 * W), dtype=dtype, device="cuda")
        wide[:, :, ::2] = c.masks.cuda().to(dtype)
        view = wide[:, :, ::2]
        assert not view.is_contiguous()
        assert torch.equal(_accumulate(c, masks=view), ref), dtype
    hwn = c.masks.permute(1, 2, 0).contiguous().cuda()                  # stored [H,W,n]
    assert torch.equal(_accumulate(c, masks=hwn.permute(2, 0, 1)), ref)
    for goal in (c.goal_cat, None, 40):
        empty = accumulate_instances(torch.zeros((0, H, W), dtype=torch.bool).cuda(), torch.zeros(0, dtype=torch.long).cuda(),
                                     torch.zeros(0).cuda(), c.n_cats, c.thr, c.goal_thr, goal).cpu()
        assert empty.shape == (H, W, c.n_cats + 1) and torch.equal(empty, torch.zeros(H, W, c.n_cats + 1))


def _seg_accumulate_raw(c, out, n_cats=None):
    """``peanut_seg_accumulate`` itself, on an output tensor the test owns."""
    from peanut_amd import _lib
    lib = _lib.load()
    masks = c.masks.cuda().view(torch.uint8).contiguous()
    classes = c.classes.to(torch.int32).cuda()
    scores = c.scores.cuda()
    H, W = masks.shape[1:]
    rc = lib.peanut_seg_accumulate(masks.data_ptr(), classes.data_ptr(), scores.data_ptr(), len(classes), H, W,
                                   c.n_cats if n_cats is None else n_cats, c.thr, c.goal_thr, -1 if c.goal_cat is None else c.goal_cat,
                                   out.data_ptr(), _lib.current_stream_ptr(out.device))
    torch.cuda.synchronize()
    return rc


def test_accumulate_refuses_zero_and_32_categories():
    from peanut_amd import _lib
    c = fg.categories(9)
    H, W = fg.ACC_HW
    out = torch.full((H, W, 34), SENTINEL, device="cuda")             # would hold 33 + 1 channels, were a launch made
    for n_cats in (0, 32, -1, 33):
        assert _seg_accumulate_raw(c, out, n_cats=n_cats) == EINVAL, n_cats
        assert b"1 <= n_cats <= 31" in _lib.load().peanut_last_error()
    assert bool((out == SENTINEL).all())
    for n_cats in (0, 32):
        with pytest.raises(_lib.PeanutHipError):
            _accumulate(SimpleNamespace(**{**vars(c), "n_cats": n_cats}))
    assert _seg_accumulate_raw(c, out[..., :10].contiguous()) == 0    # the same call with n_cats = 9 is taken


@pytest.mark.parametrize("shape", fg.STRIDE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_accumulate_pixel_loop_writes_every_pixel_with_its_own_value(shape):
    """524 800 pixels against the 2048-workgroup cap (the last 512 are a second trip of the grid-stride loop) and 300 pixels in
    two ragged workgroups: masks that are a function of the pixel index, an output that starts as NaN."""
    H, W = shape
    c = fg.stride(H, W)
    ref = fg.case_ref(c)
    out = torch.full((H, W, c.n_cats + 1), float("nan"), device="cuda")
    assert _seg_accumulate_raw(c, out) == 0
    got = out.cpu()
    assert not bool(torch.isnan(got).any()), f"{int(torch.isnan(got).any(-1).sum())} pixels unwritten"
    assert torch.equal(got, ref)
    assert torch.equal(_accumulate(c), ref)
