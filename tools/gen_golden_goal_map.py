"""Writes tests/golden/goal_map_golden.npz: what the reference's OWN ``Agent_State.update_goal_map``
(nav/agent/agent_state.py:418-446) returns on the cases of tests/goal_map_cases.py.

The reference is imported at run time as in oracle/gen_golden_goal.py (``oracle.gen_golden_agent.load_reference_agent_state``);
scikit-image is absent, so ``skimage.morphology.binary_erosion`` / ``binary_dilation`` are bound to the scipy calls scikit-image
itself makes: ``scipy.ndimage.binary_erosion(border_value=1)`` and ``binary_dilation``, default footprint.  The method is called
unbound on a stand-in object with the fields it reads.  On a CPU tensor ``.cpu().numpy()`` shares memory, so the reference's
``cat_semantic_scores[cat_semantic_scores > 0] = 1.`` rewrites its own ``local_map``: every call gets a fresh clone, and only
``goal_map`` / ``found_goal`` are recorded.

Needs the reference checkout (it does not travel with the tests; the .npz does).

    python -m tools.gen_golden_goal_map
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch
from scipy import ndimage as ndi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import goal_map_cases as gmc                      # noqa: E402
from oracle import gen_golden_agent               # noqa: E402


def generate():
    Agent_State = gen_golden_agent.load_reference_agent_state()
    import agent.agent_state as ras               # the reference module: bind its third-party names
    ras.skimage.morphology.binary_erosion = lambda image: ndi.binary_erosion(image, border_value=1)
    ras.skimage.morphology.binary_dilation = lambda image: ndi.binary_dilation(image)
    cases = gmc.all_cases()
    out = {"names": np.array([c["name"] for c in cases]), "found_goal": np.zeros(len(cases), np.int64)}
    n_found = 0
    for i, c in enumerate(cases):
        lm = c["local_map"]
        pos = lm[lm != 0]
        assert lm.min() >= 0 and (pos.size == 0 or (pos.min() >= gmc.LOW and pos.max() <= 1)), c["name"]
        st = types.SimpleNamespace(local_w=lm.shape[1], local_h=lm.shape[2], local_map=torch.from_numpy(lm.copy()).clone(),
                                   global_goals=[[c["goal"][0], c["goal"][1]]], goal_cat=c["cn"] - 4,
                                   args=types.SimpleNamespace(only_explore=0 if c["detect"] else 1, goal_erode=c["n_erode"]))
        Agent_State.update_goal_map(st, {"goal_name": "chair" if c["morph"] else "tv_monitor"})
        gm = np.asarray(st.goal_map)
        assert gm.shape == lm.shape[1:] and np.isin(gm, (0, 1)).all()
        mine, found = gmc.goal_map_ref(lm, c["cn"], c["morph"], c["n_erode"], c["detect"], c["goal"])
        assert found == st.found_goal and np.array_equal(mine, gm.astype(np.uint8)), c["name"]
        out[f"goal_map/{c['name']}"] = gm.astype(np.uint8)
        out["found_goal"][i] = int(st.found_goal)
        out[f"local_map/{c['name']}"] = lm
        out[f"params/{c['name']}"] = np.array([c["cn"], c["morph"], c["n_erode"], c["detect"], *c["goal"]], np.int64)
        n_found += int(st.found_goal)
        print(f"[goal_map] {c['name']:24s} found {int(st.found_goal)}  cells {int(gm.sum())}")
    path = gmc.GOLDEN
    np.savez_compressed(path, **out)
    print(f"[goal_map] {len(cases)} cases, {n_found} found -> {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    generate()
