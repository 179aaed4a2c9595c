"""Cases for the per-frame glue kernels at their decision boundaries (test infrastructure, importable without a GPU): the
observation formatting (``csrc/preprocess.hip``: ``Agent_Helper._preprocess_obs`` / ``_preprocess_depth``, reference
agent_helper.py:175-217) and the per-instance mask accumulation (``csrc/seg_accum.hip`` and its second copy in
``paste_accumulate_kernel``, ``csrc/rcnn_post.hip``: ``SemanticPredMaskRCNN.get_prediction``, reference segmentation.py:47-60).

Both are rules made of comparisons, so every case puts a value ON a comparison: a column that is invalid to exactly 90 %, a
depth of exactly ``0.99f``, a score that is the fp32 nearest to a threshold.  Every builder returns its inputs together with a
dict of what it claims to contain; tests/test_frame_glue_cpu.py proves the claims and shows that each neighbouring rule
(``>=`` for ``>``, the statistics over the sampled rows, float64 gates, ...) changes the expected output of a named case;
tests/test_frame_glue_gpu.py holds the device to the references bit for bit.

The reference side is not rewritten here:

* preprocess  ``oracle.agent_ref.preprocess_obs_ref`` (``preprocess_ref`` below only calls it the way the older tests do);
* accumulation  ``accumulate_ref``: the loop of segmentation.py:47-60 on CPU torch tensors.  It has to stay on torch: the reference
  compares a 0-dim float32 tensor with a Python float and torch does that in float32 (``torch.tensor(np.float32(0.95)) < 0.95`` is
  False: the instance is kept), where ``float(np.float32(0.95)) < 0.95`` is True.  A NumPy or float64 restatement is wrong exactly
  at the boundary.

NaN and negative depth are left out: the simulator's depth lies in [0, 1], and ``fmaxf`` (the kernel's column maximum) and
``ndarray.max`` (the reference's) differ on NaN.  ``-0.0`` is in: it equals 0 on both sides and counts as invalid.
"""
from types import SimpleNamespace

import numpy as np
import torch

F32 = np.float32


def below(x):
    """The float32 next to float32(x) towards -inf."""
    return np.nextafter(F32(x), F32(-np.inf))


def above(x):
    """The float32 next to float32(x) towards +inf."""
    return np.nextafter(F32(x), F32(np.inf))


def triple(x):
    """(predecessor, float32 nearest to x, successor)."""
    return below(x), F32(x), above(x)


# =================================================================================================================================
# preprocess
# =================================================================================================================================
FAR = F32(0.99)              # agent_helper.py:209: depth > 0.99 is too far
TOP = F32(0.9)               # the largest valid depth the boundary columns hold: the column-maximum fill differs visibly from 100
DENORMAL = np.float32(1.401298464324817e-45)      # 2^-149
KERNEL_THREADS = 128         # blockDim of preprocess_obs_kernel: H or H // ds above it gives a loop its second stride


def sampled_rows(H, ds):
    return np.arange(ds // 2, H, ds)


def at_count(H):
    """The largest number of invalid rows whose share is not above 0.9 (36 of 40: exactly 0.9)."""
    return (9 * H) // 10


def boundary_column(H, ds, count, placement, rng, top=TOP):
    """A depth column with exactly ``count`` invalid rows: ``placement`` 'on' puts them on the sampled rows first, 'off' on the
    skipped rows first.  The valid rows hold values in [0.1, 0.85) and one ``top``, on a skipped row wherever one is valid."""
    samp = sampled_rows(H, ds)
    skip = np.setdiff1d(np.arange(H), samp)
    order = np.concatenate([samp, skip] if placement == "on" else [skip, samp])
    col = rng.uniform(0.1, 0.85, size=H).astype(F32)
    col[order[:count]] = 0.0
    valid = order[count:]
    if len(valid):
        skipped_valid = [r for r in valid if r not in set(samp.tolist())]
        col[(skipped_valid or valid.tolist())[0]] = top
    return col


# label -> (count as a function of H, placement)
BOUNDARY_COLUMNS = {
    "below_on": (lambda H: at_count(H) - 1, "on"), "below_off": (lambda H: at_count(H) - 1, "off"),
    "at_on": (lambda H: at_count(H), "on"), "at_off": (lambda H: at_count(H), "off"),
    "above_on": (lambda H: at_count(H) + 1, "on"), "above_off": (lambda H: at_count(H) + 1, "off"),
    "none": (lambda H: 0, "on"), "all_but_one": (lambda H: H - 1, "on"), "all": (lambda H: H, "on"),
}
MEAN90_COLUMNS = list(BOUNDARY_COLUMNS)
CARRIED = ["at_on", "above_on", "above_off", "at_off", "below_on", "all_but_one"]     # what the other cases carry of mean90


def make_frame(name, H, W, ds, ncat, columns, seed=0, min_depth=0.5, max_depth=5.0, extra=None):
    """A frame (rgb uint8 [H,W,3], depth float32 [H,W,1], sem float32 [H,W,ncat], args) whose SOURCE columns
    ``ds // 2 + j * ds`` hold the named ``columns`` (as many as fit, at positions shuffled by ``seed``); the other columns are
    valid to ~90 %.  ``extra(depth, free_source_columns, rng) -> claims`` writes a case's own columns."""
    rng = np.random.RandomState(1000 + seed)
    depth = rng.uniform(0.1, 0.85, size=(H, W)).astype(F32)
    depth[rng.uniform(size=(H, W)) < 0.1] = 0.0
    rgb = rng.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
    rgb[ds // 2, ds // 2] = (0, 255, 128)                               # a sampled pixel with both ends of the range
    sem = (rng.standard_normal(size=(H, W, ncat)) * 3.0).astype(F32)   # arbitrary floats: the kernel copies, it does not test
    src = (np.arange(ds // 2, W, ds))[rng.permutation(W // ds)].tolist()
    claims = dict(name=name, H=H, W=W, ds=ds, ncat=ncat, columns={})
    if extra is not None:
        claims.update(extra(depth, src, rng))
    for label in columns:
        if not src:
            break
        count_of, placement = BOUNDARY_COLUMNS[label]
        count = max(0, min(H, count_of(H)))
        i = src.pop(0)
        depth[:, i] = boundary_column(H, ds, count, placement, rng)
        claims["columns"][label] = dict(col=i, count=count, placement=placement)
    args = SimpleNamespace(env_frame_width=W, frame_width=W // ds, min_depth=min_depth, max_depth=max_depth)
    return SimpleNamespace(name=name, rgb=rgb, depth=depth[:, :, None].copy(), sem=sem, args=args, claims=claims)


def mean90(seed=0, min_depth=0.5, max_depth=5.0, name=None):
    """40 x 48, ds = 4: source columns with 35, 36 and 37 invalid rows of 40 (36 / 40 is 0.9 exactly), each placed on and off the
    ten sampled rows, and columns with 0, 39 and 40 invalid rows."""
    return make_frame(name or f"mean90[{seed}]", 40, 48, 4, 10, MEAN90_COLUMNS, seed, min_depth, max_depth)


def _far_columns(depth, src, rng):
    H = depth.shape[0]
    ds = 4
    rows = sampled_rows(H, ds)
    lo, at, hi = triple(FAR)
    c_triple, c_special, c_fill_at, c_fill_above = (src.pop(0) for _ in range(4))
    depth[:, c_triple] = rng.uniform(0.1, 0.85, size=H).astype(F32)
    depth[rows[:3], c_triple] = (lo, at, hi)
    depth[:, c_special] = rng.uniform(0.1, 0.85, size=H).astype(F32)
    depth[rows[:3], c_special] = (F32(1.0), F32(-0.0), DENORMAL)
    depth[:, c_fill_at] = boundary_column(H, ds, at_count(H) + 1, "on", rng, top=at)       # fill = 0.99f: survives
    depth[:, c_fill_above] = boundary_column(H, ds, at_count(H) + 1, "on", rng, top=hi)    # fill = next float up: too far -> 100
    return dict(far=dict(triple=c_triple, special=c_special, fill_at=c_fill_at, fill_above=c_fill_above,
                         rows=rows[:3].tolist()))


def far099(seed=0):
    """40 x 48, ds = 4: 0.99f and its two float32 neighbours on sampled rows; 1.0, -0.0 and the smallest denormal; a mostly
    invalid column whose maximum (on a skipped row) is exactly 0.99f and one whose maximum is the next float up."""
    return make_frame(f"far099[{seed}]", 40, 48, 4, 10, CARRIED[:4], seed, extra=_far_columns)


# (H, W, ds, ncat): what the geometry is for
GEOMETRIES = [
    (516, 8, 4, 10),      # h = 129: the second stride of the output loop (and H > 128: of the statistics loop)
    (130, 6, 1, 21),      # both loops stride raggedly (130 = 128 + 2), ds // 2 = 0
    (260, 6, 2, 31),      # h = 130, H = 260 = 2 * 128 + 4
    (4, 8, 4, 1),         # h = 1
    (12, 20, 4, 10),      # H < 128: most threads idle
    (12, 20, 4, 1), (12, 20, 4, 21), (12, 20, 4, 31),
]


def geometry(H, W, ds, ncat):
    return make_frame(f"geometry[{H}x{W}/{ds},ncat={ncat}]", H, W, ds, ncat, CARRIED, seed=H + ncat)


RANGES = [(0.1, 10.0), (0.3, 3.7), (0.5, 5.0)]     # the first two: min_d * 100.0 or max_d - min_d is not a float32


def depth_range(min_depth, max_depth):
    """The mean90 frame under another depth range."""
    return mean90(0, min_depth, max_depth, name=f"range[{min_depth},{max_depth}]")


def preprocess_cases():
    """Every single-frame case, by name."""
    frames = [mean90(), far099()] + [geometry(*g) for g in GEOMETRIES] + [depth_range(*r) for r in RANGES]
    return {f.name: f for f in frames}


def preprocess_ref(fr):
    """``oracle.agent_ref.preprocess_obs_ref`` on a frame, called as tests/test_agent_gpu.py calls it: float32 [4+ncat, h, w]."""
    from oracle.agent_ref import preprocess_obs_ref
    return preprocess_obs_ref(fr.rgb.astype(np.float32), fr.depth.copy(), fr.sem, fr.args).astype(np.float32)


def preprocess_forms(fr, device="cpu"):
    """name -> (rgb, depth, sem) torch tensors on ``device`` holding the frame in the forms the wrapper accepts: depth [H,W,1],
    [H,W] and a non-contiguous slice of a wider tensor; rgb and sem as non-contiguous views."""
    H, W, ncat = fr.claims["H"], fr.claims["W"], fr.claims["ncat"]
    rgb, depth, sem = (torch.from_numpy(v).to(device) for v in (fr.rgb, fr.depth, fr.sem))
    wide = torch.full((H, W + 5), 0.77, dtype=torch.float32, device=device)
    wide[:, 3:3 + W] = depth[:, :, 0]
    wide1 = torch.full((H, W + 2, 3), 0.31, dtype=torch.float32, device=device)
    wide1[:, 1:1 + W, 1] = depth[:, :, 0]
    rgb5 = torch.full((H, W, 5), 77, dtype=torch.uint8, device=device)
    rgb5[:, :, 1:4] = rgb
    sem_chw = sem.permute(2, 0, 1).contiguous()
    forms = {
        "depth_hw1": (rgb, depth, sem),
        "depth_hw": (rgb, depth[:, :, 0].contiguous(), sem),
        "depth_slice": (rgb, wide[:, 3:3 + W], sem),
        "depth_slice_hw1": (rgb, wide1[:, 1:1 + W, 1:2], sem),
        "rgb_view": (rgb5[:, :, 1:4], depth, sem),
        "sem_view": (rgb, depth, sem_chw.permute(1, 2, 0)),
    }
    return forms


BATCH_PERM = [5, 12, 0, 9, 14, 3, 7, 1, 15, 10, 2, 13, 6, 11, 4, 8]


def batch_frames(E):
    """E frames of one shape (40 x 48, ds 4, ncat 10, range 0.5 / 5.0) taken from the cases above: E = 1 and E = 16 =
    PEANUT_MAP_MAX_BATCH are the ends of what ``peanut_preprocess_obs_batch`` accepts."""
    frames = [f(s) for s in range(8) for f in (mean90, far099)]
    assert 1 <= E <= len(frames)
    return frames[:E]


# =================================================================================================================================
# accumulation
# =================================================================================================================================
THR, GOAL_THR = 0.95, 0.985       # nav/arguments.py: sem_pred_prob_thr, goal_thr -- Python floats, as the reference holds them
ACC_HW = (8, 16)
GRID_CAP, BLOCK = 2048, 256       # peanut_seg_accumulate: at most 2048 workgroups of 256 threads


def accumulate_ref(masks, classes, scores, n_cats, thr, goal_thr, goal_cat):
    """segmentation.py:47-60 on CPU torch tensors (the loop is the whole algorithm): ``scores[j]`` stays a 0-dim tensor, so the
    gates are evaluated in the scores' dtype as torch does for the reference."""
    H, W = masks.shape[1:]
    ref = torch.zeros(H, W, n_cats + 1)
    for j, cls in enumerate(classes.numpy()):
        if cls in range(n_cats):
            if scores[j] < thr:
                continue
            if cls == goal_cat and scores[j] < goal_thr:
                continue
            ref[:, :, cls] += masks[j] * 1.
    return ref


def _acc_case(name, masks, classes, scores, n_cats, thr, goal_thr, goal_cat, **claims):
    return SimpleNamespace(name=name, masks=masks, classes=torch.as_tensor(classes, dtype=torch.int64),
                           scores=torch.as_tensor(np.asarray(scores, dtype=np.float32)), n_cats=n_cats, thr=thr, goal_thr=goal_thr,
                           goal_cat=goal_cat, claims=dict(name=name, **claims))


def case_ref(c):
    return accumulate_ref(c.masks, c.classes, c.scores, c.n_cats, c.thr, c.goal_thr, c.goal_cat)


GATE_N_CATS = 9
GATE_GOAL, GATE_OTHER, GATE_ABSENT = 3, 5, 7
GATE_SCORES = list(triple(THR)) + list(triple(GOAL_THR)) + [F32(0.0), F32(1.0), F32(np.nan)]
GATE_GOALS = {"present": GATE_GOAL, "absent": GATE_ABSENT, "none": None, "out_of_range": GATE_N_CATS + 2}
GATE_THRESHOLDS = {"default": (THR, GOAL_THR), "goal_below": (GOAL_THR, THR), "equal": (THR, THR)}


def gates(goal="present", thresholds="default"):
    """Every score of GATE_SCORES once in the goal class and once in another class, plus confident instances of classes -1,
    n_cats - 1, n_cats and n_cats + 5 (+ 2 when that is the goal).  Every instance has its own random mask, so a wrong decision
    about any one of them shows."""
    n_cats = GATE_N_CATS
    classes, scores = [], []
    for cls in (GATE_GOAL, GATE_OTHER):
        classes += [cls] * len(GATE_SCORES)
        scores += GATE_SCORES
    edge_classes = [-1, n_cats - 1, n_cats, n_cats + 5, n_cats + 2]
    classes += edge_classes
    scores += [F32(0.999)] * len(edge_classes)
    order = np.random.RandomState(7).permutation(len(classes))          # instance order is not class order
    classes = [classes[i] for i in order]
    scores = [scores[i] for i in order]
    g = torch.Generator().manual_seed(11)
    masks = torch.rand((len(classes),) + ACC_HW, generator=g) > 0.5
    thr, goal_thr = GATE_THRESHOLDS[thresholds]
    return _acc_case(f"gates[{goal},{thresholds}]", masks, classes, scores, n_cats, thr, goal_thr, GATE_GOALS[goal],
                     goal_class=GATE_GOAL, other_class=GATE_OTHER, edge_classes=edge_classes)


COUNT_PIXEL = (3, 5)


def counts(as_uint8=False):
    """100 instances of class 2 interleaved with 50 of class 6; every mask covers COUNT_PIXEL, which reads 100.0 / 50.0.  The
    masks as bool, or as uint8 holding 0 and 1 (what ``accumulate_instances`` documents)."""
    n, n_cats = 150, 9
    classes = [6 if j % 3 == 2 else 2 for j in range(n)]
    g = torch.Generator().manual_seed(13)
    masks = torch.rand((n,) + ACC_HW, generator=g) > 0.7
    masks[:, COUNT_PIXEL[0], COUNT_PIXEL[1]] = True
    if as_uint8:
        masks = masks.to(torch.uint8)
    return _acc_case(f"counts[{'uint8' if as_uint8 else 'bool'}]", masks, classes, [F32(0.99)] * n, n_cats, THR, GOAL_THR, None,
                     per_class={2: 100, 6: 50})


CATEGORY_COUNTS = [1, 9, 21, 31]       # the entry accepts 1..31; the 25-channel configuration uses 21


def categories(n_cats):
    """An instance in class 0, one in class n_cats - 1 and one in class n_cats (dropped: channel n_cats stays zero)."""
    classes = [0, n_cats - 1, n_cats, 0]
    g = torch.Generator().manual_seed(17 + n_cats)
    masks = torch.rand((len(classes),) + ACC_HW, generator=g) > 0.5
    return _acc_case(f"categories[{n_cats}]", masks, classes, [F32(0.99)] * len(classes), n_cats, THR, GOAL_THR, n_cats - 1)


STRIDE_SHAPES = [(2, 262400), (1, 300)]     # 524 800 pixels: 512 past the 2048-workgroup cap; 300: a ragged single workgroup


def stride_masks(H, W, n=3):
    """Masks that are a function of the pixel index alone: bit 29 + j of the low 32 bits of p * 2654435761, which depends on every
    bit of p below it -- a pixel written with the value of pixel p - 256 or p - 2048 * 256 shows."""
    p = np.arange(H * W, dtype=np.uint64)
    hashed = (p * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    m = np.stack([((hashed >> np.uint64(29 + j)) & np.uint64(1)).astype(bool) for j in range(n)])
    return torch.from_numpy(m.reshape(n, H, W))


def stride(H, W):
    """n = 3, n_cats = 2: classes 1, 0, 1, all kept."""
    return _acc_case(f"stride[{H}x{W}]", stride_masks(H, W), [1, 0, 1], [F32(0.99)] * 3, 2, THR, GOAL_THR, 0, pixels=H * W)


def accumulation_cases():
    """Every case ``accumulate_instances`` is held to the loop on, by name (the stride cases apart: they go through the C entry
    with an output that starts as NaN)."""
    cs = [gates(g, "default") for g in GATE_GOALS] + [gates("present", t) for t in ("goal_below", "equal")]
    cs += [gates("absent", "equal"), counts(False), counts(True)] + [categories(k) for k in CATEGORY_COUNTS]
    return {c.name: c for c in cs}
