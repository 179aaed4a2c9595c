"""tests/frame_glue_cases.py without a GPU: every case holds what it claims, and every case separates the reference's rule from
its neighbours.

The second half restates the two rules with switches (``preprocess_variant``, ``accumulate_variant``), shows that the restatement
with every switch off IS the reference on every case, and then turns one switch on at a time: ``>= 0.9``, ``>= 0.99``, the mean
or the maximum over the sampled rows only, ``(max_d - min_d) * 100.0`` folded into one constant, ``<= thr``, ``<= goal_thr``, the
gates in float64.  Each must move the expected output of the cases named next to it -- a kernel that implements the variant then
fails tests/test_frame_glue_gpu.py on those cases -- and every case must be moved by some variant: one that is not has stopped
doing its job."""
import numpy as np
import pytest
import torch

import frame_glue_cases as fg

F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases hold what they claim
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fg.preprocess_cases()))
def test_boundary_columns_have_the_stated_counts(name):
    fr = fg.preprocess_cases()[name]
    H, ds = fr.claims["H"], fr.claims["ds"]
    rows = fg.sampled_rows(H, ds)
    d = fr.depth[:, :, 0]
    assert fr.rgb.dtype == np.uint8 and fr.depth.dtype == np.float32 and fr.sem.dtype == np.float32
    assert fr.depth.shape == (H, fr.claims["W"], 1) and fr.sem.shape == (H, fr.claims["W"], fr.claims["ncat"])
    assert not np.isnan(d).any() and d.min() >= 0.0
    assert fr.claims["columns"], "every case carries columns of mean90"
    for label, c in fr.claims["columns"].items():
        col = d[:, c["col"]]
        assert c["col"] % ds == ds // 2, "a source column of the subsampling"
        assert int((col == 0).sum()) == c["count"], label
        on_sampled = int((col[rows] == 0).sum())
        if c["placement"] == "on":
            assert on_sampled == min(c["count"], len(rows)), label
        else:
            assert on_sampled == max(0, c["count"] - (H - len(rows))), label
        valid = col[col != 0]
        if len(valid):
            assert valid.max() == fg.TOP and valid.max() <= F32(0.9)
            if len(np.setdiff1d(np.flatnonzero(col != 0), rows)):
                assert int(np.argmax(col)) not in rows.tolist(), f"{label}: the column maximum sits on a skipped row"
    samp = fr.rgb[ds // 2::ds, ds // 2::ds]
    assert samp.min() == 0 and samp.max() == 255
    assert len(np.unique(fr.sem)) > 2, "sem holds arbitrary floats"


def test_mean90_hits_the_threshold_exactly_and_from_both_sides():
    fr = fg.mean90()
    cols = fr.claims["columns"]
    assert set(cols) == set(fg.MEAN90_COLUMNS)
    assert {k: v["count"] for k, v in cols.items()} == dict(below_on=35, below_off=35, at_on=36, at_off=36, above_on=37,
                                                            above_off=37, none=0, all_but_one=39, all=40)
    rows = fg.sampled_rows(40, 4)
    assert len(rows) == 10
    d = fr.depth[:, :, 0]
    share = {k: (float(np.mean(d[:, v["col"]] == 0)), float(np.mean(d[rows, v["col"]] == 0))) for k, v in cols.items()}
    assert share["at_on"][0] == 0.9 and share["at_off"][0] == 0.9 and not share["at_on"][0] > 0.9      # np.mean gives 0.9 itself
    # the share over the sampled rows lies on the other side of 0.9 than the share over the column, in both directions
    for k in ("below_on", "at_on"):
        assert share[k][0] <= 0.9 < share[k][1] == 1.0
    for k in ("above_off",):
        assert share[k][1] == 0.7 <= 0.9 < share[k][0]
    for k in ("below_on", "below_off", "at_on", "at_off", "above_on", "above_off", "all_but_one", "all"):
        assert (d[rows, cols[k]["col"]] == 0).any(), "an invalid pixel on a sampled row: the fill reaches the output"
    # where the fill is the column maximum and no sampled row is valid, the maximum over the sampled rows is 0
    for k in ("above_on", "all_but_one"):
        assert d[rows, cols[k]["col"]].max() == 0.0 and d[:, cols[k]["col"]].max() == fg.TOP


def test_far099_values_sit_on_sampled_rows():
    fr = fg.far099()
    far = fr.claims["far"]
    rows = fg.sampled_rows(40, 4)
    d = fr.depth[:, :, 0]
    lo, at, hi = fg.triple(0.99)
    assert lo < at < hi and at == F32(0.99) and np.nextafter(lo, F32(1)) == at and np.nextafter(at, F32(1)) == hi
    assert set(far["rows"]) <= set(rows.tolist())
    assert d[far["rows"], far["triple"]].tolist() == [lo, at, hi]
    sp = d[far["rows"], far["special"]]
    assert sp[0] == 1.0 and sp[1] == 0.0 and np.signbit(sp[1]) and 0.0 < sp[2] == fg.DENORMAL < np.finfo(np.float32).tiny
    for key, top in (("fill_at", at), ("fill_above", hi)):
        col = d[:, far[key]]
        assert np.mean(col == 0) > 0.9 and col.max() == top and (col[rows] == 0).all()
    ref = fg.preprocess_ref(fr)[3]
    j = {k: far[k] // 4 for k in ("triple", "special", "fill_at", "fill_above")}
    kept = F32(50.0) + (F32(0.99) * F32(4.5)) * F32(100.0)
    gone = F32(50.0) + (F32(100.0) * F32(4.5)) * F32(100.0)
    assert ref[:3, j["triple"]].tolist() == [F32(50.0) + (lo * F32(4.5)) * F32(100.0), kept, gone]
    assert ref[:3, j["special"]].tolist() == [gone, gone, F32(50.0)]       # 1.0 too far, -0.0 invalid, the denormal 0 cm past 50
    assert (ref[:, j["fill_at"]] == kept).all() and (ref[:, j["fill_above"]] == gone).all()


def test_geometries_reach_the_loop_strides():
    seen = set()
    for H, W, ds, ncat in fg.GEOMETRIES:
        assert H % ds == 0 and W % ds == 0
        seen.add((H > fg.KERNEL_THREADS, H // ds > fg.KERNEL_THREADS, H // ds == 1, ds // 2 == 0, ncat))
    assert (516, 8, 4) in [g[:3] for g in fg.GEOMETRIES] and 516 // 4 == fg.KERNEL_THREADS + 1
    assert any(s[1] for s in seen) and any(s[2] for s in seen) and any(s[3] for s in seen) and any(not s[0] for s in seen)
    assert {g[3] for g in fg.GEOMETRIES} == {1, 10, 21, 31}
    assert 130 % fg.KERNEL_THREADS and 260 % fg.KERNEL_THREADS and (260 // 2) % fg.KERNEL_THREADS      # ragged strides


def test_range_constants_are_inexact_in_float32():
    inexact = []
    for lo, hi in fg.RANGES:
        base, span = lo * 100.0, hi - lo
        inexact.append(float(F32(base)) != base or float(F32(span)) != span)
    assert inexact == [True, True, False]
    assert [fg.depth_range(*r).args.min_depth for r in fg.RANGES] == [0.1, 0.3, 0.5]
    assert np.array_equal(fg.depth_range(0.5, 5.0).depth, fg.mean90().depth)


def test_wrapper_forms_are_the_same_frame_in_other_strides():
    fr = fg.mean90()
    forms = fg.preprocess_forms(fr)
    rgb0, depth0, sem0 = forms["depth_hw1"]
    assert depth0.shape == (40, 48, 1) and forms["depth_hw"][1].shape == (40, 48)
    for name, (rgb, depth, sem) in forms.items():
        assert torch.equal(rgb, rgb0) and torch.equal(sem, sem0) and torch.equal(depth.reshape(40, 48), depth0.reshape(40, 48)), name
    assert not forms["depth_slice"][1].is_contiguous() and not forms["depth_slice_hw1"][1].is_contiguous()
    assert not forms["rgb_view"][0].is_contiguous() and not forms["sem_view"][2].is_contiguous()


def test_batch_frames_share_a_shape_and_differ():
    frames = fg.batch_frames(16)
    assert len(frames) == 16 and len(fg.batch_frames(1)) == 1
    assert {(f.depth.shape, f.sem.shape, f.args.frame_width, f.args.min_depth, f.args.max_depth) for f in frames} == \
        {((40, 48, 1), (40, 48, 10), 12, 0.5, 5.0)}
    refs = [fg.preprocess_ref(f) for f in frames]
    assert all(not np.array_equal(refs[a], refs[b]) for a in range(16) for b in range(a))
    assert sorted(fg.BATCH_PERM) == list(range(16)) and all(p != i for i, p in enumerate(fg.BATCH_PERM))


def test_score_triples_bracket_their_thresholds_in_float32():
    for t in (fg.THR, fg.GOAL_THR):
        lo, at, hi = fg.triple(t)
        assert lo < at < hi and at == F32(t)
        s = torch.tensor([lo, at, hi])
        assert [bool(s[k] < t) for k in range(3)] == [True, False, False]            # torch: float32 -- `at` is kept
        assert float(lo) < t and float(hi) > t                                      # ... and the triple brackets t itself
    assert float(F32(fg.THR)) < fg.THR, "float32(0.95) lies below 0.95: a float64 gate drops the instance torch keeps"
    c = fg.gates()
    for cls in (c.claims["goal_class"], c.claims["other_class"]):
        have = c.scores[c.classes == cls].numpy()
        for v in fg.GATE_SCORES:
            assert (np.isnan(have).sum() == 1) if np.isnan(v) else (have == v).sum() == 1
    assert set(c.claims["edge_classes"]) >= {-1, c.n_cats - 1, c.n_cats, c.n_cats + 5}
    assert all((c.classes == k).any() for k in c.claims["edge_classes"])
    assert fg.GATE_GOALS["present"] in c.classes.tolist() and fg.GATE_GOALS["absent"] not in c.classes.tolist()
    assert fg.GATE_GOALS["none"] is None and fg.GATE_GOALS["out_of_range"] >= c.n_cats
    assert fg.GATE_GOALS["out_of_range"] in c.classes.tolist()
    assert all(bool(m.any()) for m in c.masks), "a dropped instance always shows"
    t = fg.GATE_THRESHOLDS
    assert t["goal_below"][1] < t["goal_below"][0] and t["equal"][0] == t["equal"][1]
    assert all(isinstance(v, float) for pair in t.values() for v in pair)


def test_counts_categories_and_stride_claims():
    c = fg.counts()
    assert sum(1 for k in c.classes.tolist() if k == 2) == 100 and len(c.classes) == 150
    assert c.classes.tolist()[:6] == [2, 2, 6, 2, 2, 6], "interleaved"
    ref = fg.case_ref(c)
    y, x = fg.COUNT_PIXEL
    assert ref[y, x, 2] == 100.0 and ref[y, x, 6] == 50.0 and ref.max() == 100.0
    u = fg.counts(as_uint8=True)
    assert u.masks.dtype == torch.uint8 and set(u.masks.unique().tolist()) == {0, 1} and torch.equal(fg.case_ref(u), ref)
    for k in fg.CATEGORY_COUNTS:
        c = fg.categories(k)
        ref = fg.case_ref(c)
        assert ref.shape == fg.ACC_HW + (k + 1,) and float(ref[..., k].abs().max()) == 0.0
        assert float(ref[..., 0].max()) > 0 and float(ref[..., k - 1].max()) > 0
    assert fg.CATEGORY_COUNTS == [1, 9, 21, 31]
    (H, W), (h1, w1) = fg.STRIDE_SHAPES
    assert H * W == fg.GRID_CAP * fg.BLOCK + 512 and h1 * w1 == 300
    m = fg.stride_masks(H, W).reshape(3, -1)
    tail = slice(fg.GRID_CAP * fg.BLOCK, H * W)
    for shift in (fg.BLOCK, fg.GRID_CAP * fg.BLOCK, fg.GRID_CAP):
        assert not torch.equal(m[:, tail], m[:, tail.start - shift:tail.stop - shift]), "the tail differs from the pixels a wrong stride reads"
    assert 0.3 < float(m.float().mean()) < 0.7


# ---------------------------------------------------------------------------------------------------------------------------------
# the rules with their neighbours
# ---------------------------------------------------------------------------------------------------------------------------------
def preprocess_variant(fr, mean_ge=False, far_ge=False, mean_sampled=False, max_sampled=False, one_constant=False):
    """agent_helper.py:175-217 once more, in NumPy, with one switch per neighbouring rule."""
    a = fr.args
    ds = a.env_frame_width // a.frame_width
    depth = fr.depth[:, :, 0] * 1
    rows = fg.sampled_rows(depth.shape[0], ds)
    for i in range(depth.shape[1]):
        invalid = depth[:, i] == 0.
        share = np.mean(invalid[rows]) if mean_sampled else np.mean(invalid)
        if (share >= 0.9) if mean_ge else (share > 0.9):
            depth[:, i][invalid] = depth[rows, i].max() if max_sampled else depth[:, i].max()
        else:
            depth[:, i][invalid] = 100.0
    depth[(depth >= 0.99) if far_ge else (depth > 0.99)] = 0.
    depth[depth == 0] = 100.0
    if one_constant:
        depth = a.min_depth * 100.0 + depth * ((a.max_depth - a.min_depth) * 100.0)
    else:
        depth = a.min_depth * 100.0 + depth * (a.max_depth - a.min_depth) * 100.0
    rgb, sem = fr.rgb.astype(np.float32), fr.sem
    if ds != 1:
        rgb, depth, sem = (v[ds // 2::ds, ds // 2::ds] for v in (rgb, depth, sem))
    return np.concatenate((rgb, depth[:, :, None], sem), axis=2).transpose(2, 0, 1).astype(np.float32)


def accumulate_variant(c, le_thr=False, le_goal=False, f64=False):
    """segmentation.py:47-60 once more, with one switch per neighbouring rule."""
    H, W = c.masks.shape[1:]
    ref = torch.zeros(H, W, c.n_cats + 1)
    for j, cls in enumerate(c.classes.numpy()):
        if cls in range(c.n_cats):
            sc = float(c.scores[j]) if f64 else c.scores[j]
            if (sc <= c.thr) if le_thr else (sc < c.thr):
                continue
            if cls == c.goal_cat and ((sc <= c.goal_thr) if le_goal else (sc < c.goal_thr)):
                continue
            ref[:, :, cls] += c.masks[j] * 1.
    return ref


# variant -> the cases it has to move (it may move more)
PREPROCESS_VARIANTS = {
    "mean_ge": ["mean90[0]", "far099[0]", "geometry[130x6/1,ncat=21]", "geometry[260x6/2,ncat=31]", "range[0.1,10.0]"],
    "far_ge": ["far099[0]"],
    "mean_sampled": ["mean90[0]", "far099[0]", "geometry[516x8/4,ncat=10]", "geometry[260x6/2,ncat=31]", "geometry[4x8/4,ncat=1]",
                     "geometry[12x20/4,ncat=10]"],
    "max_sampled": ["mean90[0]", "far099[0]", "geometry[516x8/4,ncat=10]", "geometry[260x6/2,ncat=31]", "geometry[12x20/4,ncat=21]"],
    "one_constant": ["range[0.1,10.0]", "range[0.3,3.7]"],
}
ACCUMULATE_VARIANTS = {
    "le_thr": ["gates[present,default]", "gates[none,default]", "gates[present,goal_below]", "gates[present,equal]"],
    "le_goal": ["gates[present,default]", "gates[present,equal]"],
    "f64": ["gates[present,default]", "gates[absent,default]", "gates[none,default]", "gates[out_of_range,default]"],
}


def test_the_restatements_with_every_switch_off_are_the_references():
    for name, fr in fg.preprocess_cases().items():
        assert np.array_equal(preprocess_variant(fr), fg.preprocess_ref(fr)), name
    for name, c in fg.accumulation_cases().items():
        assert torch.equal(accumulate_variant(c), fg.case_ref(c)), name


@pytest.mark.parametrize("variant", list(PREPROCESS_VARIANTS))
def test_each_preprocess_variant_moves_its_cases(variant):
    cases = fg.preprocess_cases()
    for name in PREPROCESS_VARIANTS[variant]:
        fr = cases[name]
        ref, var = fg.preprocess_ref(fr), preprocess_variant(fr, **{variant: True})
        assert not np.array_equal(var, ref), f"{variant} leaves {name} unchanged"
        assert np.array_equal(np.delete(var, 3, axis=0), np.delete(ref, 3, axis=0)), "only the depth channel moves"


@pytest.mark.parametrize("variant", list(ACCUMULATE_VARIANTS))
def test_each_accumulation_variant_moves_its_cases(variant):
    cases = fg.accumulation_cases()
    for name in ACCUMULATE_VARIANTS[variant]:
        c = cases[name]
        assert not torch.equal(accumulate_variant(c, **{variant: True}), fg.case_ref(c)), f"{variant} leaves {name} unchanged"


def test_every_boundary_case_is_moved_by_some_variant():
    """mean90, far099, every geometry and range case, and every gates case: none is a bystander.  (counts, categories and
    stride hold no value on a gate: they pin the instance-to-channel mapping, the channel range and the pixel loop.)"""
    for name, fr in fg.preprocess_cases().items():
        ref = fg.preprocess_ref(fr)
        moved = [v for v in PREPROCESS_VARIANTS if not np.array_equal(preprocess_variant(fr, **{v: True}), ref)]
        assert moved, name
    for name, c in fg.accumulation_cases().items():
        if name.startswith("gates"):
            ref = fg.case_ref(c)
            moved = [v for v in ACCUMULATE_VARIANTS if not torch.equal(accumulate_variant(c, **{v: True}), ref)]
            assert moved, name


def test_the_float64_gate_is_wrong_exactly_at_the_boundary():
    """What the module docstring warns of, as numbers: torch keeps the instance whose score is float32(0.95), float64 drops it."""
    at = torch.tensor(F32(0.95))
    assert not bool(at < 0.95) and float(at) < 0.95
    c = fg.gates("none", "default")
    diff = fg.case_ref(c) - accumulate_variant(c, f64=True)
    j = [k for k in range(len(c.scores)) if c.scores[k] == F32(0.95) and int(c.classes[k]) in (c.claims["goal_class"], c.claims["other_class"])]
    want = torch.zeros_like(diff)
    for k in j:
        want[:, :, int(c.classes[k])] += c.masks[k] * 1.
    assert len(j) == 2 and torch.equal(diff, want)
