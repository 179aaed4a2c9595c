"""``peanut_plan_mark`` / ``peanut_plan_mark_batch`` (csrc/plan.hip) at their smallest shapes: windows of 2, 3 and 8 cells in full
maps of 4 .. 16, in every corner and in the middle, on maps pre-filled with a random 0 / 1 pattern.  The whole of both maps is compared
bit for bit with a NumPy restatement that uses real Python slices (``mat[x - 1:x + 1, y - 1:y + 1] = 1``: nothing along an axis whose
coordinate is 0).  Every refusal leaves every map untouched."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import plan_cases as pc
from peanut_amd import _lib
from peanut_amd.agent_helper import plan_mark, plan_mark_batch

pytestmark = pytest.mark.gpu


def restate(visited, collision, lmb, last_start, start, cells):
    """agent_helper.py:278-280 and :315 on NumPy copies."""
    visited, collision = visited.copy(), collision.copy()
    gx1, gx2, gy1, gy2 = lmb
    mat = visited[gx1:gx2, gy1:gy2]
    for x, y in pc.line(last_start, start):
        mat[x - 1:x + 1, y - 1:y + 1] = 1
    for r, c in cells:
        collision[r, c] = 1
    return visited, collision


def windows(m, full):
    """The m x m window in the four corners and in the middle of the full map."""
    lo, hi, mid = 0, full - m, (full - m) // 2
    return [(a, a + m, b, b + m) for a, b in ((lo, lo), (lo, hi), (hi, lo), (hi, hi), (mid, mid))]


def filled(rng, full, E=1):
    return [(rng.random((full, full)) < 0.3).astype(np.uint8) for _ in range(2 * E)]


def run(marks_np):
    """E episodes given as NumPy maps -> the maps after one launch, and the restatement's."""
    dev = [(torch.from_numpy(v).cuda(), torch.from_numpy(c).cuda()) + tuple(rest) for v, c, *rest in marks_np]
    if len(dev) == 1:
        plan_mark(*dev[0])
    else:
        plan_mark_batch(dev)
    torch.cuda.synchronize()
    got = [(d[0].cpu().numpy(), d[1].cpu().numpy()) for d in dev]
    want = [restate(*mk) for mk in marks_np]
    return got, want


def assert_same(got, want, what):
    for e, ((gv, gc), (wv, wc)) in enumerate(zip(got, want)):
        assert np.array_equal(gv, wv), f"{what}: visited_vis of episode {e} differs at {np.argwhere(gv != wv)[:4].tolist()}"
        assert np.array_equal(gc, wc), f"{what}: collision_map of episode {e} differs at {np.argwhere(gc != wc)[:4].tolist()}"


@pytest.mark.parametrize("m, full", [(2, 4), (2, 5), (3, 7), (3, 4), (8, 16), (8, 11)])
def test_single_mark_equals_python_slices_in_every_corner(m, full):
    rng = np.random.default_rng(100 * m + full)
    cells_of = lambda n: [(int(r), int(c)) for r, c in rng.integers(0, full, (n, 2))]
    for w, lmb in enumerate(windows(m, full)):
        if m <= 3 and w == 0:             # every (last_start, start) pair of the window
            pairs = [((a, b), (c, d)) for a in range(m) for b in range(m) for c in range(m) for d in range(m)]
        else:                             # its corners and edges, and a few random pairs
            pairs = [((0, 0), (m - 1, m - 1)), ((m - 1, 0), (0, m - 1)), ((0, m - 1), (0, 0)), ((m - 1, m - 1), (m - 1, m - 1)), ((0, 0), (0, 0))]
            pairs += [(tuple(int(v) for v in rng.integers(0, m, 2)), tuple(int(v) for v in rng.integers(0, m, 2))) for _ in range(4)]
        for k, (last, start) in enumerate(pairs):
            v, c = filled(rng, full)
            n = (0, 1, 28, 5)[k % 4]
            cells = cells_of(n) if n != 28 else cells_of(24) + [(0, 0), (full - 1, full - 1), (0, full - 1), (full - 1, 0)]
            got, want = run([(v, c, lmb, last, start, cells)])
            assert_same(got, want, f"m {m} full {full} lmb {lmb} {last} -> {start}, {n} cells")


def test_zero_maps_show_the_empty_slices():
    """On zero maps the rule is visible: a walk along row 0 of the window marks nothing, one along row 1 marks rows 0 and 1, and
    column 0 of the window is only ever marked from column 1."""
    full, lmb, m = 12, (2, 10, 3, 11), 8
    z = lambda: np.zeros((full, full), np.uint8)
    got, want = run([(z(), z(), lmb, (0, 0), (0, m - 1), [])])
    assert_same(got, want, "row 0")
    assert got[0][0].sum() == 0
    got, want = run([(z(), z(), lmb, (1, 1), (1, m - 1), [])])
    assert_same(got, want, "row 1")
    assert got[0][0].sum() == 2 * m and got[0][0][2:4, 3:11].all()
    got, want = run([(z(), z(), lmb, (m - 1, 0), (m - 1, 0), [(11, 11)])])
    assert got[0][0].sum() == 0 and got[0][1].sum() == 1 and got[0][1][11, 11] == 1


@pytest.mark.parametrize("E", [1, 3, 16])
def test_batched_mark_equals_single_calls(E):
    """Different windows, window sizes and cell counts 0 / 1 / 28 per episode in one launch: every map equals the restatement (which
    test_single_mark... holds the single call to) and the single call itself."""
    rng = np.random.default_rng(7 + E)
    full = 16
    marks = []
    for e in range(E):
        m = (2, 3, 8)[e % 3]
        lmb = windows(m, full)[e % 5]
        v, c = filled(rng, full)
        n = (0, 1, 28)[e % 3]
        cells = [(int(r), int(cc)) for r, cc in rng.integers(0, full, (n, 2))]
        last, start = tuple(int(x) for x in rng.integers(0, m, 2)), tuple(int(x) for x in rng.integers(0, m, 2))
        if e == 1:
            last, start = (0, m - 1), (m - 1, 0)
        marks.append((v, c, lmb, last, start, cells))
    got, want = run(marks)
    assert_same(got, want, f"batch of {E}")
    singles = [run([mk])[0][0] for mk in marks]
    assert_same(got, singles, f"batch of {E} against single calls")


def _refusals(full, m):
    ok = dict(lmb=(1, 1 + m, 2, 2 + m), last=(0, 1), start=(m - 1, 0), cells=[(0, 0)])
    bad = [dict(lmb=(1, 2, 2, 3), last=(0, 0), start=(0, 0)), dict(lmb=(1, 1 + m, 2, 1 + m)), dict(lmb=(full - m + 1, full + 1, 2, 2 + m)),
           dict(start=(m, 0)), dict(last=(0, -1)), dict(cells=[(0, 0)] * 29), dict(cells=[(full, 0)]), dict(cells=[(3, 3), (0, -1)])]
    return ok, [dict(ok, **b) for b in bad]


def test_every_refusal_leaves_every_map_untouched():
    full, m = 9, 3
    rng = np.random.default_rng(3)
    ok, bad = _refusals(full, m)
    maps_np = filled(rng, full, E=3)
    maps = [torch.from_numpy(a).cuda() for a in maps_np]
    mk = lambda e, d: (maps[2 * e], maps[2 * e + 1], d["lmb"], d["last"], d["start"], d["cells"])
    for b in bad:
        with pytest.raises((_lib.PeanutHipError, ValueError)):
            plan_mark(*mk(0, b))
        for slot in range(3):
            with pytest.raises((_lib.PeanutHipError, ValueError)):
                plan_mark_batch([mk(e, b if e == slot else ok) for e in range(3)])
    for shared in ([mk(0, ok), mk(0, ok)], [mk(0, ok), (maps[2], maps[1], ok["lmb"], ok["last"], ok["start"], ok["cells"])],
                   [(maps[0], maps[0], ok["lmb"], ok["last"], ok["start"], ok["cells"])], [mk(e % 3, ok) for e in range(17)]):
        with pytest.raises((_lib.PeanutHipError, ValueError)):
            plan_mark_batch(shared)
    torch.cuda.synchronize()
    for t, a in zip(maps, maps_np):
        assert np.array_equal(t.cpu().numpy(), a)
    # ... and the same maps take a good call afterwards
    plan_mark_batch([mk(e, ok) for e in range(3)])
    torch.cuda.synchronize()
    for e in range(3):
        wv, wc = restate(maps_np[2 * e], maps_np[2 * e + 1], ok["lmb"], ok["last"], ok["start"], ok["cells"])
        assert np.array_equal(maps[2 * e].cpu().numpy(), wv) and np.array_equal(maps[2 * e + 1].cpu().numpy(), wc)
