"""Cases and NumPy / scipy restatement of the reference's ``Agent_State.update_goal_map`` (nav/agent/agent_state.py:418-446)
for tests/test_goal_map_cpu.py and tests/test_goal_map_gpu.py.

``goal_map_ref`` restates the method statement by statement, with scikit-image's ``binary_erosion`` / ``binary_dilation``
written as the scipy calls they make (``scipy.ndimage.binary_erosion(border_value=1)`` / ``binary_dilation``, default footprint:
the 4-connected cross).  tests/golden/goal_map_golden.npz holds what the reference's OWN method returned on the same cases
(tools/gen_golden_goal_map.py); the CPU test holds the restatement to it, the GPU tests hold the kernels to it.

Every map value is 0 or lies in [2^-10, 1]: for such values the sign of `sum(planes 4:10) - own plane` is the same in every
summation order, so the comparison of rule 3 cannot depend on how torch orders its reduction."""
from __future__ import annotations

import os

import numpy as np
from scipy import ndimage as ndi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "goal_map_golden.npz")
M = 40              # not a multiple of the kernel's 32-cell tile, and it crosses a 32-boundary
M_RANDOM = 72
C = 14              # 4 + num_sem_categories
LOW = np.float32(2.0 ** -10)
N_RANDOM = 12


def goal_map_ref(local_map, cn, morph, n_erode, detect, goal):
    """(goal_map uint8 [m, m], found_goal) of agent_state.py:423-446 for ``local_map`` [C, m, m] (fp32, non-negative)."""
    lm = np.asarray(local_map, dtype=np.float32)
    goal_map = np.zeros(lm.shape[1:], np.uint8)
    goal_map[goal[0], goal[1]] = 1
    found = 0
    if detect and lm[cn].sum() != 0:
        s = lm[cn] > 0
        if morph:
            for _ in range(n_erode):
                s = ndi.binary_erosion(s, border_value=1)
            s = ndi.binary_dilation(s)
        total = lm[4]
        for ch in range(5, min(10, lm.shape[0])):
            total = total + lm[ch]                  # fp32, ((((c4 + c5) + c6) + c7) + c8) + c9
        s = s & ((total - lm[cn]) == 0)
        if s.any():
            goal_map = s.astype(np.uint8)
            found = 1
    return goal_map, found


def _case(name, lm, cn=4, morph=1, n_erode=3, detect=1, goal=(5, 7)):
    return dict(name=name, local_map=lm, cn=cn, morph=morph, n_erode=n_erode, detect=detect, goal=(int(goal[0]), int(goal[1])))


def _blank(m=M):
    return np.zeros((C, m, m), np.float32)


def _block(r0, r1, c0, c1, cn=4, value=1.0, m=M):
    lm = _blank(m)
    lm[cn, r0:r1, c0:c1] = value
    return lm


def named_cases():
    """The hand-made cases at m = 40; EXPECT lists found and the number of set cells of each."""
    out = [
        _case("sq7_interior", _block(10, 17, 10, 17)),
        _case("sq6_vanishes", _block(10, 16, 10, 16)),
        _case("sq7_across_32", _block(29, 36, 29, 36, value=0.5)),
        _case("top_border_4x7", _block(0, 4, 10, 17)),
        _case("corner_4x4", _block(0, 4, 0, 4)),
        _case("far_corner", _block(36, 40, 33, 40)),
        _case("whole_map", _block(0, M, 0, M, value=0.25)),
        _case("sq7_erode0", _block(10, 17, 10, 17), n_erode=0),
        _case("sq7_erode1", _block(10, 17, 10, 17), n_erode=1),
        _case("sq17_erode8", _block(11, 28, 20, 37), n_erode=8),
        _case("sq16_erode8", _block(11, 27, 20, 36), n_erode=8),
    ]
    lm = _blank()
    rr, cc = np.mgrid[0:M, 0:M]
    lm[4][np.abs(rr - 20) + np.abs(cc - 21) <= 3] = 0.75
    out.insert(2, _case("diamond3", lm))
    lm = _blank()
    lm[4, 33, 2] = LOW
    out.append(_case("tv_single_cell", lm, morph=0))
    lm = _block(10, 17, 10, 17)
    lm[6, 8:19, 8:19] = 0.5
    out.append(_case("overlap_whole", lm))
    lm = _block(10, 17, 10, 27)                     # 7 x 17 -> a 1 x 11 line (row 13, columns 13..23), dilated: 35 cells
    lm[9, 0:M, 20:M] = LOW                          # another category claims the columns from 20 on: 8 + 7 + 7 cells stay
    out.append(_case("overlap_part", lm))
    lm = _block(10, 17, 10, 17)
    lm[5, 9, 13] = LOW                              # (9, 13) is added by the dilation only, and category 5 holds it
    out.append(_case("dilated_cell_masked", lm, n_erode=0))
    lm = _block(10, 17, 10, 17, cn=7)
    lm[4, 30:37, 2:9] = 1.0                         # another category's blob elsewhere must not be reported
    out.append(_case("cn7", lm, cn=7))
    out.append(_case("cn12_outside_4_10", _block(10, 17, 10, 17, cn=12), cn=12))   # sum(4:10) - own < 0 everywhere: never found
    out.append(_case("detect_off", _block(10, 17, 10, 17), detect=0))
    out.append(_case("goal_first_cell", _blank(), goal=(0, 0)))
    out.append(_case("goal_last_cell", _blank(), goal=(M - 1, M - 1)))
    return out


# name -> (found, set cells of goal_map)
EXPECT = {
    "sq7_interior": (1, 5), "sq6_vanishes": (0, 1), "diamond3": (1, 5), "sq7_across_32": (1, 5), "top_border_4x7": (1, 4),
    "corner_4x4": (1, 3), "far_corner": (1, 9), "whole_map": (1, M * M), "sq7_erode0": (1, 77), "sq7_erode1": (1, 45),
    "sq17_erode8": (1, 5), "sq16_erode8": (0, 1), "tv_single_cell": (1, 1), "overlap_whole": (0, 1), "overlap_part": (1, 22),
    "dilated_cell_masked": (1, 76), "cn7": (1, 5), "cn12_outside_4_10": (0, 1), "detect_off": (0, 1), "goal_first_cell": (0, 1),
    "goal_last_cell": (0, 1),
}
# name -> the set cells themselves, where the issue names them
EXPECT_CELLS = {
    "sq7_interior": [(12, 13), (13, 12), (13, 13), (13, 14), (14, 13)],
    "sq7_across_32": [(31, 32), (32, 31), (32, 32), (32, 33), (33, 32)],
    "top_border_4x7": [(0, 12), (0, 13), (0, 14), (1, 13)],
    "corner_4x4": [(0, 0), (0, 1), (1, 0)],
    "sq6_vanishes": [(5, 7)],
    "tv_single_cell": [(33, 2)],
    "goal_first_cell": [(0, 0)],
    "goal_last_cell": [(M - 1, M - 1)],
}


def random_cases(seed=20418, n=N_RANDOM, m=M_RANDOM):
    """Seeded blob maps at m = 72: blobs of the goal category (even cases: at least one large enough to survive the erosions; odd
    cases: only small ones, which vanish), blobs of other categories over and beside them, single noisy cells."""
    rng = np.random.RandomState(seed)
    out = []
    for k in range(n):
        lm = _blank(m)
        cn = int(rng.randint(4, 10))
        n_erode = int(rng.randint(1, 4))
        morph = 0 if k % 6 == 5 else 1
        def blob(ch, lo, hi):
            h, w = rng.randint(lo, hi + 1, size=2)
            r0, c0 = rng.randint(-3, m - 2, size=2)
            r0c, c0c = max(r0, 0), max(c0, 0)
            shape = lm[ch, r0c:r0 + h, c0c:c0 + w].shape
            lm[ch, r0c:r0 + h, c0c:c0 + w] = rng.uniform(LOW, 1.0, size=shape).astype(np.float32)
        small = 2 * n_erode
        for _ in range(rng.randint(2, 6)):
            blob(cn, 1, small)
        if k % 2 == 0:
            for _ in range(rng.randint(1, 3)):
                blob(cn, 2 * n_erode + 3, 20)
        others = [ch for ch in range(4, C) if ch != cn]
        for _ in range(rng.randint(2, 6)):
            blob(others[rng.randint(len(others))], 2, 9 if k % 2 == 0 else 30)
        for _ in range(30):
            lm[rng.randint(4, C), rng.randint(m), rng.randint(m)] = rng.uniform(LOW, 1.0)
        if k % 2 == 1 and morph == 0:               # without erosion a small blob is found unless another category covers it
            lm[others[0]][lm[cn] > 0] = LOW
        lm[lm > 1] = 1.0
        out.append(_case(f"random{k:02d}", lm, cn=cn, morph=morph, n_erode=n_erode, goal=(rng.randint(m), rng.randint(m))))
    return out


def all_cases():
    return named_cases() + random_cases()


def load_golden():
    """name -> (goal_map uint8, found_goal) as the reference's own update_goal_map returned them."""
    with np.load(GOLDEN) as z:
        names = [str(s) for s in z["names"]]
        return {n: (z[f"goal_map/{n}"], int(z["found_goal"][i])) for i, n in enumerate(names)}
