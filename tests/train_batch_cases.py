"""Augmented training batches (ABI 25): the cases, inputs and the float64 restatement of the rule shared by
tools/gen_golden_train_batch.py, tests/test_train_batch_cpu.py and tests/test_train_batch_gpu.py.  Importable without a GPU and
without the reference.

The goldens (tests/golden/train_batch_golden.npz, written by tools/gen_golden_train_batch.py) are the reference's OWN ``Resize``,
``Pad``, ``RandomCrop``, ``RandomFlip`` and ``RandomRotate`` (mmseg/datasets/pipelines/transforms.py, unmodified) under
``np.random.seed(seed)`` on these cases; the rotation itself is scipy's ``affine_transform(mode='grid-constant')`` (cv2 is absent
where the fixtures are made).  The file holds data only: the uint8 sequences (``sequences`` rebuilds them from their seeds), the
seeds, the draws the pipeline made and its outputs."""
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "train_batch_golden.npz")

# ---- golden cases: the reference's pipeline under a seed -----------------------------------------------------------------------
# map (W, H), channels C, target channels K, the T of the sequences a case's samples come from in turn (sample i: sequence
# i % len(T), snapshot i % T), pad / crop (rows, columns), the RandomFlip direction, RandomRotate's prob, samples n, seed.
OFF_CASES = {   # rotation off (RandomRotate prob 0: the angle is still drawn)
    "tall":  dict(map=(5, 7), C=6, K=2, T=(3,), pad=(8, 9), crop=(6, 6), direction="horizontal", n=10, seed=3),    # the crop is taller than the map
    "one":   dict(map=(9, 11), C=6, K=2, T=(2,), pad=(12, 12), crop=(1, 1), direction="vertical", n=8, seed=1),     # crop 1 x 1
    "tight": dict(map=(12, 16), C=5, K=1, T=(2,), pad=(12, 16), crop=(12, 16), direction="horizontal", n=4, seed=2),  # pad = map, crop = pad: margin 0
    "m47":   dict(map=(47, 47), C=14, K=6, T=(3,), pad=(50, 49), crop=(45, 47), direction="horizontal", n=4, seed=4),  # scalar path, misaligned planes
    "m48":   dict(map=(48, 48), C=14, K=6, T=(3, 5), pad=(56, 56), crop=(48, 48), direction="horizontal", n=6, seed=5),  # vector path; two T in one call
    "rect":  dict(map=(40, 56), C=14, K=6, T=(2,), pad=(44, 60), crop=(32, 48), direction="vertical", n=4, seed=6),   # a rectangular crop
}
ON_CASES = {    # rotation on, angles uniform in +-180
    "rot_odd":  dict(map=(24, 24), C=6, K=2, T=(3,), pad=(30, 30), crop=(21, 23), direction="horizontal", n=4, seed=11, rotate_prob=1.0),
    "rot_even": dict(map=(24, 28), C=6, K=2, T=(2,), pad=(28, 32), crop=(20, 28), direction="vertical", n=4, seed=12, rotate_prob=1.0),
    "rot_some": dict(map=(16, 16), C=5, K=1, T=(2,), pad=(20, 20), crop=(16, 12), direction="horizontal", n=8, seed=13, rotate_prob=0.5),  # the angle is drawn either way
}
FLIP_PROB = 0.5
DEGREE = 180

# ---- rotation at stated angles, held to the restatement on the GPU ----------------------------------------------------------
ANGLES = (0.0, 90.0, -90.0, 180.0, 17.0, -142.137, 0.001, 179.999)
ANGLE_SHAPES = {    # both sides of one parity: at +-90 degrees a mixed pair puts every nearest tap on a half-integer
    "odd":  dict(map=(47, 47), C=14, K=6, T=3, pad=(60, 64), crop=(45, 47)),     # scalar stores, more than one tile both ways
    "even": dict(map=(48, 48), C=14, K=6, T=3, pad=(64, 96), crop=(36, 72)),     # vector stores, two tiles across, three down
}
TIE_MARGIN = 1e-9


def pipeline(case):
    """The ``train_pipeline`` list of a golden case, in the shape of nav/pred_model_cfg.py:47-56."""
    return [
        dict(type="LoadMapFromFile"),
        dict(type="Resize", img_scale=None, ratio_range=(1.0, 1.0)),
        dict(type="Pad", size=tuple(case["pad"]), pad_val=0, seg_pad_val=0),
        dict(type="RandomCrop", crop_size=tuple(case["crop"]), cat_max_ratio=1.0),
        dict(type="RandomFlip", flip_ratio=FLIP_PROB, direction=case["direction"]),
        dict(type="RandomRotate", prob=case.get("rotate_prob", 0.0), degree=DEGREE, pad_val=0, seg_pad_val=0),
        dict(type="DefaultFormatBundle"),
        dict(type="Collect", keys=["img", "gt_semantic_seg"]),
    ]


def make_sequence(T, C, shape, seed):
    """uint8 [T, C, W, H]: sparse maps with bytes over the whole range, channel 1 (explored) zero on about 60 % of the cells."""
    rng = np.random.RandomState(seed)
    size = (T, C) + tuple(shape)
    maps = (rng.uniform(0, 1, size) ** 2 * 256).astype(np.uint8) * (rng.uniform(0, 1, size) > 0.7)
    maps[:, 1] *= (rng.uniform(0, 1, (T,) + tuple(shape)) > 0.6)
    return np.ascontiguousarray(maps.astype(np.uint8))


def sequences(case, seed_base=None):
    seed_base = 1000 * case["seed"] if seed_base is None else seed_base
    Ts = case["T"] if isinstance(case["T"], tuple) else (case["T"],)
    return [make_sequence(T, case["C"], case["map"], seed_base + k) for k, T in enumerate(Ts)]


def sample_sources(case):
    """[(sequence index, t_idx)] of the case's samples."""
    Ts = case["T"]
    return [(i % len(Ts), i % Ts[i % len(Ts)]) for i in range(case["n"])]


def rotation_terms(angle_deg):
    a = math.radians(float(angle_deg))
    return math.cos(a), math.sin(a)


def restate(maps, t, off_r, off_c, flip, rotate, angle, pad, crop, K):
    """The rule in float64 on one sample -> dict(img float64 [C,Sr,Sc], gt uint8 [K,Sr,Sc], near (ys + 0.5, xs + 0.5) or None).
    With rotation off ``img`` holds float32(byte) / float32(255) exactly."""
    T, C, W, H = maps.shape
    Sr, Sc = crop
    assert pad[0] >= W and pad[1] >= H and 0 <= off_r <= pad[0] - Sr and 0 <= off_c <= pad[1] - Sc
    val = (maps[t].astype(np.float32) / np.float32(255.0)).astype(np.float64)
    tgt = maps[-1, 4:4 + K] * (maps[t, 1] == 0)

    def tap(yi, xi):
        """-> (valid, r, q) with r, q clipped into the map where invalid"""
        ok = (yi >= 0) & (yi < Sr) & (xi >= 0) & (xi < Sc)
        if flip == 1:
            xi = Sc - 1 - xi
        elif flip == 2:
            yi = Sr - 1 - yi
        r, q = yi + off_r, xi + off_c
        ok = ok & (r < W) & (q < H) & (r >= 0) & (q >= 0)
        return ok, np.clip(r, 0, W - 1), np.clip(q, 0, H - 1)

    y, x = np.mgrid[0:Sr, 0:Sc]
    if not rotate:
        ok, r, q = tap(y, x)
        return dict(img=val[:, r, q] * ok, gt=(tgt[:, r, q] * ok).astype(np.uint8), near=None)
    cy, cx = (Sr - 1) / 2.0, (Sc - 1) / 2.0
    c, s = rotation_terms(angle)
    ys = c * (y - cy) - s * (x - cx) + cy
    xs = s * (y - cy) + c * (x - cx) + cx
    y0, x0 = np.floor(ys), np.floor(xs)
    fy, fx = ys - y0, xs - x0
    y0, x0 = y0.astype(np.int64), x0.astype(np.int64)
    img = np.zeros((C, Sr, Sc), np.float64)
    for (dy, dx), w in (((0, 0), (1 - fy) * (1 - fx)), ((0, 1), (1 - fy) * fx), ((1, 0), fy * (1 - fx)), ((1, 1), fy * fx)):
        ok, r, q = tap(y0 + dy, x0 + dx)
        img += w * (val[:, r, q] * ok)
    ok, r, q = tap(np.floor(ys + 0.5).astype(np.int64), np.floor(xs + 0.5).astype(np.int64))
    return dict(img=img, gt=(tgt[:, r, q] * ok).astype(np.uint8), near=(ys + 0.5, xs + 0.5))


def tie_distance(near):
    """How close the nearest-tap coordinates of a sample come to a half-integer (in ``near`` = coordinate + 0.5: to an integer)."""
    return min(float(np.abs(v - np.rint(v)).min()) for v in near)


def angle_params(angles, shape, seed=0):
    """Parameter rows (plain tuples: off_r, off_c, flip, rotate, angle) for the stated angles: offsets and flips from a seeded
    stream, the first sample at offset 0 without a flip, the second at the full margin."""
    rng = np.random.RandomState(seed)
    mr, mc = shape["pad"][0] - shape["crop"][0], shape["pad"][1] - shape["crop"][1]
    rows = []
    for i, a in enumerate(angles):
        off = (0, 0) if i == 0 else (mr, mc) if i == 1 else (int(rng.randint(0, mr + 1)), int(rng.randint(0, mc + 1)))
        rows.append((off[0], off[1], 0 if i == 0 else int(rng.randint(0, 3)), 1, float(a)))
    return rows


# ---- what peanut_mapseq_train_batch refuses (PEANUT_EINVAL, nothing enqueued) ----------------------------------------------------
def train_desc(img=4096, gt=8192, maps=4096, stream=None, **over):
    """A valid peanut_mapseq_train_t for the sizes of case "tall" (by default on fake addresses that no refused call dereferences), then
    edited: ``over`` names fields of the descriptor or of its samples; ``n_samples`` the length of the sample array."""
    import ctypes as C

    from peanut_amd import _lib
    f = dict(size=C.sizeof(_lib.MapSeqTrainC), B=1, C=6, W=5, H=7, pad_r=8, pad_c=9, S_r=6, S_c=6, K=2, img=img, gt=gt, stream=stream)
    s = dict(maps=maps, T=3, t_idx=0, off_r=0, off_c=0, flip=0, rotate=0, cos_t=1.0, sin_t=0.0)
    n = over.pop("n_samples", 1)
    for k in list(over):
        if k in s:
            s[k] = over.pop(k)
    f.update(over)
    arr = (_lib.MapSeqAugC * n)()
    for a in arr:
        for k, v in s.items():
            setattr(a, k, v)
    d = _lib.MapSeqTrainC(f["size"], f["B"], f["C"], f["W"], f["H"], f["pad_r"], f["pad_c"], f["S_r"], f["S_c"], f["K"], 0,
                          arr if f.get("samples", 1) else None, f["img"], f["gt"], f["stream"])
    d._keep = arr
    return d


REFUSALS = {
    "size": dict(size=8), "null samples": dict(samples=0), "null img": dict(img=None), "null maps": dict(maps=None),
    "B 0": dict(B=0), "B 65": dict(B=65, n_samples=65),
    "C 4": dict(C=4, K=1), "K 0": dict(K=0), "K 3": dict(K=3),
    "pad rows < map": dict(pad_r=4, S_r=4), "pad columns < map": dict(pad_c=6),
    "crop rows > pad": dict(S_r=9), "crop columns > pad": dict(S_c=10), "crop 0": dict(S_r=0),
    "off_r < 0": dict(off_r=-1), "off_r > margin": dict(off_r=3), "off_c < 0": dict(off_c=-1), "off_c > margin": dict(off_c=4),
    "t_idx < 0": dict(t_idx=-1), "t_idx = T": dict(t_idx=3),
    "flip -1": dict(flip=-1), "flip 3": dict(flip=3),
    "cos nan": dict(cos_t=float("nan")), "sin inf": dict(sin_t=float("inf")), "not a unit vector": dict(cos_t=1.0, sin_t=1e-4),
    "zero vector": dict(cos_t=0.0, sin_t=0.0),
}
