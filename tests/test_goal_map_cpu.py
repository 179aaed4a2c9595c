"""The goal-map fixture (tests/golden/goal_map_golden.npz: the reference's own ``Agent_State.update_goal_map`` through scipy's
morphology, tools/gen_golden_goal_map.py) against the restatement the GPU tests travel with (tests/goal_map_cases.py), the
fixture's own claims, and the binding of the two new calls."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import goal_map_cases as gmc      # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return gmc.load_golden()


def test_restatement_equals_the_reference_on_every_case(golden):
    cases = gmc.all_cases()
    assert sorted(golden) == sorted(c["name"] for c in cases) and len(cases) == len(gmc.EXPECT) + gmc.N_RANDOM
    with np.load(gmc.GOLDEN) as z:
        for c in cases:
            # the builders still make the maps the reference saw
            assert np.array_equal(z[f"local_map/{c['name']}"], c["local_map"]), c["name"]
            assert list(z[f"params/{c['name']}"]) == [c["cn"], c["morph"], c["n_erode"], c["detect"], *c["goal"]], c["name"]
    for c in cases:
        before = c["local_map"].copy()
        gm, found = gmc.goal_map_ref(c["local_map"], c["cn"], c["morph"], c["n_erode"], c["detect"], c["goal"])
        want, want_found = golden[c["name"]]
        assert gm.dtype == np.uint8 and found == want_found and np.array_equal(gm, want), c["name"]
        assert np.array_equal(before, c["local_map"]), c["name"]                 # the restatement leaves its input alone


def test_map_values_are_zero_or_in_the_stated_range():
    for c in gmc.all_cases():
        lm = c["local_map"]
        pos = lm[lm != 0]
        assert lm.dtype == np.float32 and (pos >= gmc.LOW).all() and (pos <= 1).all(), c["name"]


def test_named_cases_hold_what_they_claim(golden):
    for c in gmc.named_cases():
        gm, found = golden[c["name"]]
        want_found, want_cells = gmc.EXPECT[c["name"]]
        assert (found, int(gm.sum())) == (want_found, want_cells), c["name"]
        assert gm.shape == (gmc.M, gmc.M) and np.isin(gm, (0, 1)).all()
        if c["name"] in gmc.EXPECT_CELLS:
            cells = sorted((int(r), int(q)) for r, q in zip(*np.nonzero(gm)))
            assert cells == sorted(gmc.EXPECT_CELLS[c["name"]]), c["name"]
        if not found:
            assert gm[c["goal"]] == 1                                            # one-hot at the long-term goal
    far = golden["far_corner"][0]
    assert far[0].sum() == 0 and far[:, 0].sum() == 0                            # nothing wrapped to row or column 0
    # erosion that took the outside for unset would lose these
    assert golden["top_border_4x7"][1] == 1 and golden["corner_4x4"][1] == 1


def test_random_cases_are_found_and_not_found(golden):
    found = [golden[c["name"]][1] for c in gmc.random_cases()]
    assert len(found) == gmc.N_RANDOM
    assert 3 * sum(found) >= len(found) and 3 * (len(found) - sum(found)) >= len(found)
    assert any(c["morph"] == 0 for c in gmc.random_cases())


def test_the_two_calls_are_bound_at_abi_18():
    from peanut_amd import _lib
    assert "peanut_goal_map" in _lib.SIGNATURES and "peanut_goal_map_batch" in _lib.SIGNATURES
    assert _lib.ABI_VERSION >= 18


def test_default_args_keep_the_switch_off_and_replay_names_the_goal():
    from peanut_amd.agent_state import default_args
    from peanut_amd.peanut_agent import coco_goal_names, hm3d_names, hm3d_to_coco
    a = default_args()
    assert a.goal_map is False and a.goal_erode == 3
    assert all(coco_goal_names[hm3d_to_coco[k]] == hm3d_names[k] for k in hm3d_names)
    assert "tv" in coco_goal_names[5] and sum("tv" in n for n in coco_goal_names.values()) == 1
