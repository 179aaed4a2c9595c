"""Sliding-window and flip-averaged inference (ABI 24): the cases, inputs and rule shared by tools/gen_golden_infer.py,
tests/test_infer_cpu.py and tests/test_infer_gpu.py.  Importable without a GPU and without the reference.

Weights: ``make_seeded_state_dict(PredCfg(), 0)``.  Inputs: seeded sparse maps with values in [0, 1] (``inputs``).

The goldens (tests/golden/infer_golden.npz, written by tools/gen_golden_infer.py) are the reference's own ``EncoderDecoder``
(slide_inference / inference / aug_test through ``forward_test``) on these cases."""
import os

import numpy as np
import torch

from small_map_cases import TOL  # noqa: F401  (5e-5: what the fp32 forward is held to on logits and on sigmoid outputs)

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "infer_golden.npz")

# name -> image (H, W), batch, crop (h, w), stride (h, w)
CASES = {
    "A": dict(H=41, W=53, B=3, crop=(24, 32), stride=(16, 20)),   # odd sizes (scalar path), ragged last windows shifted back; counts {1,2,3,4,6,9}
    "B": dict(H=40, W=56, B=1, crop=(24, 32), stride=(16, 24)),   # everything a multiple of 4 (vector path); counts {1,2,4}
    "C": dict(H=33, W=47, B=1, crop=(16, 16), stride=(16, 16)),   # the smallest window, no overlap but the shifted last row / column
    "D": dict(H=20, W=60, B=1, crop=(32, 24), stride=(8, 12)),    # crop taller than the image: the small patch, a 1 x 4 grid
    "E": dict(H=40, W=56, B=1, crop=(64, 64), stride=(32, 32)),   # crop >= image on both axes: one window
}
COUNTS = {"A": {1, 2, 3, 4, 6, 9}, "B": {1, 2, 4}}

# name -> flip code per image handed to forward_test (0 none, 1 horizontal, 2 vertical)
AUG_LISTS = {
    "none": (0,),
    "none_h": (0, 1),
    "two_dirs": (0, 0, 1, 2),      # MultiScaleFlipAug(flip=True, flip_direction=['horizontal', 'vertical'])
    "v": (2,),                     # one vertically flipped image, through the descriptor alone
}
FLIP_DIMS = {1: (3,), 2: (2,)}     # encoder_decoder.py:253-256
FLIP_NAMES = {1: "horizontal", 2: "vertical"}


def key(case, augs, mode="slide"):
    return f"{case}/{mode}/{augs}"


def inputs(case, seed_offset=0, channels=14):
    """float32 [B, channels, H, W]: ~30 % of the cells hold a value in [0, 1), the rest 0."""
    c = CASES[case]
    g = torch.Generator().manual_seed(1000 * c["H"] + c["W"] + 7 * (ord(case) - ord("A")) + 100003 * seed_offset)
    shape = (c["B"], channels, c["H"], c["W"])
    return (torch.rand(shape, generator=g) > 0.7).float() * torch.rand(shape, generator=g)


def flip(x, code):
    return x.flip(FLIP_DIMS[code]) if code else x


def windows(H, W, crop, stride):
    """The window loop of encoder_decoder.py:166-177 restated -> ([(y1, x1, y2, x2)] rows outer, columns inner; h_grids; w_grids)."""
    def spans(n, size, step):
        grids = max(n - size + step - 1, 0) // step + 1
        ends = [min(i * step + size, n) for i in range(grids)]
        return [(max(e - size, 0), e) for e in ends]
    rows, cols = spans(H, crop[0], stride[0]), spans(W, crop[1], stride[1])
    return [(y1, x1, y2, x2) for y1, y2 in rows for x1, x2 in cols], len(rows), len(cols)


def count_matrix(H, W, crop, stride):
    cnt = np.zeros((H, W), np.int64)
    for y1, x1, y2, x2 in windows(H, W, crop, stride)[0]:
        cnt[y1:y2, x1:x2] += 1
    return cnt


def staged_batch(x, wins, flips):
    """The staged batch in the contracted order: aug-major, then sample, then window row-major; the flip applied to the whole
    image before the windows are cut.  ``wins``: [(y1, x1, y2, x2)] of one window size."""
    return torch.cat([flip(x, f)[b:b + 1, :, y1:y2, x1:x2] for f in flips for b in range(x.shape[0]) for (y1, x1, y2, x2) in wins])


def combine(logits, wins, flips, B, H, W, slide=True):
    """The stated rule in torch's fp32 arithmetic on ``logits`` [N, K, ch, cw] (the staged order) -> [B, K, H, W]."""
    K, nw = logits.shape[1], len(wins)
    count = torch.zeros((1, 1, H, W), dtype=torch.float32, device=logits.device)
    for y1, x1, y2, x2 in wins:
        count[:, :, y1:y2, x1:x2] += 1
    out = None
    for a, f in enumerate(flips):
        if slide:
            s = torch.zeros((B, K, H, W), dtype=torch.float32, device=logits.device)
            for b in range(B):
                for i, (y1, x1, y2, x2) in enumerate(wins):
                    s[b, :, y1:y2, x1:x2] = s[b, :, y1:y2, x1:x2] + logits[(a * B + b) * nw + i]
            p = s / count
        else:
            p = logits[a * B:(a + 1) * B]
        p = flip(p, f)
        out = p if out is None else out + p
    if len(flips) > 1:      # (a tensor divisor: torch turns a division by a Python scalar into a multiplication by its reciprocal)
        out = out / torch.full((1,), float(len(flips)), dtype=torch.float32, device=logits.device)
    return out
