"""The motion planner's host side -- no GPU needed.

1. ABI 22 and its three symbols.
2. ``peanut_plan_line`` against the NumPy expression of ``vu.draw_line`` (nav/agent/utils/visualization.py:19-24) for every
   (last_start, start) pair of a 12 x 12 grid, and at large coordinates.
3. What every chain of tests/plan_cases.py claims to exercise, on the committed fixture (the reference's own ``_plan``).
4. The refusals of ``peanut_plan_mark`` / ``peanut_plan_mark_batch``: they are decided on the host before anything is enqueued, so
   they need no device (the map pointers are never dereferenced on the host).
5. ``UnTrapHelper`` and the host state machine of ``Agent_Helper`` on every chain, with the maps left out."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import plan_cases as pc
from peanut_amd import _lib, agent_helper as ahm


def test_abi_version_is_at_least_22_and_the_plan_symbols_are_bound():
    lib = _lib.load()
    assert _lib.ABI_VERSION >= 22
    assert lib.peanut_abi_version() == _lib.ABI_VERSION
    for name in ("peanut_plan_line", "peanut_plan_mark", "peanut_plan_mark_batch"):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes is not None
    assert C.sizeof(_lib.PlanMarkC) == 16 + 4 * (4 + 2 + 2 + 1 + 2 * _lib.PLAN_MAX_CELLS) + 4      # (4 bytes of tail padding)
    assert C.sizeof(_lib.PlanMapsC) == 16


def test_plan_line_equals_numpy_on_every_pair_of_a_12_grid():
    cells = [(r, c) for r in range(12) for c in range(12)]
    n = 0
    for a in cells:
        for b in cells:
            got = ahm.plan_line(a, b)
            assert got.shape == (26, 2)
            assert [tuple(p) for p in got] == pc.line(a, b), (a, b)
            n += 1
    assert n == 144 * 144


@pytest.mark.parametrize("a, b", [((0, 4095), (4095, 0)), ((4095, 4095), (0, 0)), ((1, 2), (1, 2)), ((3, 0), (0, 28)), ((12, 37), (13, 12))])
def test_plan_line_equals_numpy_at_large_cells(a, b):
    """The largest window the library takes, both directions, a point, and differences whose quotients come nearest to a half
    ((end - start) * i / 25 is never exactly one: 25 is odd)."""
    assert [tuple(p) for p in ahm.plan_line(a, b)] == pc.line(a, b)


def test_the_fixture_holds_every_chain_and_its_claims():
    golden = pc.load_golden()
    chains = pc.chains()
    assert set(golden) == set(chains) == set(pc.CLAIMS)
    for name, chain in chains.items():
        g = golden[name]
        T = len(chain["steps"])
        assert g["state"].shape == (T, len(pc.STATE)) and g["visited"].shape == g["collision"].shape == (T, pc.FULL, pc.FULL)
        assert g["visited"].dtype == g["collision"].dtype == np.uint8
        pc.CLAIMS[name](chain, g)
        # the maps only grow, and their counts are the recorded ones
        assert (np.diff(g["visited"].astype(np.int8), axis=0) >= 0).all() and (np.diff(g["collision"].astype(np.int8), axis=0) >= 0).all()
        assert [int(v) for v in g["collision"].reshape(T, -1).sum(1)] == [int(v) for v in pc.col(g["state"], "n_collision")]
        assert [int(v) for v in g["visited"].reshape(T, -1).sum(1)] == [int(v) for v in pc.col(g["state"], "n_visited")]
    assert os.path.getsize(pc.GOLDEN) < 64 * 1024
    assert {c["cfg"]["num_sem_categories"] for c in chains.values()} == {10, 17}
    assert {c["cfg"]["move_forward_after_stop"] for c in chains.values()} == {0, 1, 2}


# ---- the refusals: decided before anything is enqueued -------------------------------------------------------------------------
FAKE_A, FAKE_B, FAKE_C, FAKE_D = 0x10000000, 0x20000000, 0x30000000, 0x40000000      # never dereferenced: every call below is refused


def _maps(full=16):
    return _lib.PlanMapsC(full_w=full, full_h=full, stream=None)


def _ep(visited=FAKE_A, collision=FAKE_B, lmb=(4, 12, 4, 12), last=(1, 1), start=(2, 2), cells=()):
    ep = _lib.PlanMarkC(visited_vis=visited, collision_map=collision, n_cells=len(cells))
    ep.lmb[:], ep.last_start[:], ep.start[:] = lmb, last, start
    for k, (r, c) in enumerate(cells[:_lib.PLAN_MAX_CELLS]):
        ep.cells_rc[k][0], ep.cells_rc[k][1] = r, c
    return ep


REFUSED = {
    "null visited": dict(visited=None),
    "null collision": dict(collision=None),
    "m = 1": dict(lmb=(4, 5, 4, 5), last=(0, 0), start=(0, 0)),
    "m = 0": dict(lmb=(4, 4, 4, 4), last=(0, 0), start=(0, 0)),
    "window not square": dict(lmb=(4, 12, 4, 11)),
    "window below the map": dict(lmb=(-1, 7, 4, 12)),
    "window beyond the rows": dict(lmb=(9, 17, 4, 12)),
    "window beyond the columns": dict(lmb=(4, 12, 9, 17)),
    "start at m": dict(start=(8, 2)),
    "start negative": dict(start=(2, -1)),
    "last_start at m": dict(last=(1, 8)),
    "last_start negative": dict(last=(-1, 1)),
    "cell row at full_w": dict(cells=((16, 0),)),
    "cell column negative": dict(cells=((0, -1),)),
    "one map for both": dict(collision=FAKE_A),
    "maps overlap": dict(collision=FAKE_A + 255),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_plan_mark_refuses_before_it_enqueues(name):
    lib = _lib.load()
    maps, ep = _maps(), _ep(**REFUSED[name])
    assert lib.peanut_plan_mark(C.byref(maps), C.byref(ep)) == -2, name
    assert lib.peanut_last_error()
    # ... and as one of three episodes, in every slot: one refused episode refuses the whole call
    for slot in range(3):
        eps = (_lib.PlanMarkC * 3)(*[ep if k == slot else _ep(visited=FAKE_C + 0x1000 * k, collision=FAKE_D + 0x1000 * k) for k in range(3)])
        assert lib.peanut_plan_mark_batch(C.byref(maps), 3, eps) == -2, (name, slot)


def test_plan_mark_refuses_bad_counts_and_shared_maps():
    lib = _lib.load()
    maps = _maps()
    ep = _ep()
    ep.n_cells = _lib.PLAN_MAX_CELLS + 1
    assert lib.peanut_plan_mark(C.byref(maps), C.byref(ep)) == -2
    ep.n_cells = -1
    assert lib.peanut_plan_mark(C.byref(maps), C.byref(ep)) == -2
    assert lib.peanut_plan_mark(None, C.byref(_ep())) == -2 and lib.peanut_plan_mark(C.byref(maps), None) == -2
    good = [_ep(visited=FAKE_A + 0x1000 * k, collision=FAKE_B + 0x1000 * k) for k in range(17)]
    for E in (0, -1, 17):
        assert lib.peanut_plan_mark_batch(C.byref(maps), E, (_lib.PlanMarkC * 17)(*good)) == -2, E
    assert lib.peanut_plan_mark_batch(C.byref(maps), 2, None) == -2
    # two episodes naming the same map: as visited twice, as visited and collision, and merely overlapping
    for other in (dict(visited=FAKE_A, collision=FAKE_C), dict(visited=FAKE_C, collision=FAKE_A), dict(visited=FAKE_C, collision=FAKE_B + 100)):
        eps = (_lib.PlanMarkC * 2)(_ep(), _ep(**other))
        assert lib.peanut_plan_mark_batch(C.byref(maps), 2, eps) == -2, other
    for full in (1, 65537):
        assert lib.peanut_plan_mark(C.byref(_lib.PlanMapsC(full_w=full, full_h=16, stream=None)), C.byref(_ep())) == -2


def test_the_python_mirror_refuses_host_tensors_and_too_many_cells():
    import torch
    v, c = torch.zeros((16, 16), dtype=torch.uint8), torch.zeros((16, 16), dtype=torch.uint8)
    with pytest.raises(ValueError):
        ahm.plan_mark(v, c, (4, 12, 4, 12), (1, 1), (2, 2))
    with pytest.raises(ValueError):
        ahm.plan_mark_batch([])


# ---- the host state machine on the chains (maps left out) ----------------------------------------------------------------------
def test_untrap_helper_sequence():
    u = ahm.UnTrapHelper()
    np.random.seed(5)
    first = [u.get_action() for _ in range(30)]
    assert first == [2] * 2 + [3] * 16 + [2] * 12
    assert set(u.get_action() for _ in range(40)) == {2, 3}
    u.reset()
    assert (u.total_id, u.epi_id) == (1, 0)
    assert [u.get_action() for _ in range(30)] == [3] * 2 + [2] * 16 + [3] * 12
    u.reset(full=True)
    assert (u.total_id, u.epi_id) == (0, 0)


@pytest.mark.parametrize("name", sorted(pc.chains()))
def test_host_state_machine_follows_the_reference_on_every_chain(name):
    """``_plan_begin`` / ``_plan_end`` (everything but the two device calls) against the fixture: actions, counters, ``last_start``
    and, per step, the collision cells as the set difference of the golden maps."""
    chain, g = pc.chains()[name], pc.load_golden()[name]
    args = SimpleNamespace(**pc.cfg_args(chain["cfg"]))
    m = pc.local_size(chain["cfg"])
    maps = SimpleNamespace(shape=(pc.FULL, pc.FULL), zero_=lambda: None)
    state = SimpleNamespace(collision_map=maps, visited_vis=maps, device=None, stg=None, stg_stop=None)
    h = ahm.Agent_Helper(args, state)
    h.reset()
    np.random.seed(chain["cfg"]["seed"])
    seen = np.zeros((pc.FULL, pc.FULL), np.uint8)
    for k, s in enumerate(chain["steps"]):
        inputs = {'obstacle': np.zeros((m, m), np.float32), 'goal': np.zeros((m, m)), 'pose_pred': np.array(list(s["pose"]) + s["lmb"], np.float64),
                  'found_goal': s["found"], 'goal_name': 'chair'}
        h.timestep += 1
        step = h._plan_begin(inputs)
        action = h._plan_end(inputs, step, s["stg"], bool(s["stop"]))
        h.last_action = action
        row = [action, h.col_width, h.prev_blocked, h.forward_after_stop, h._previous_action, h.last_action, h.untrap.total_id, h.untrap.epi_id,
               h.timestep, h.last_start[0], h.last_start[1]]
        assert row == [int(v) for v in g["state"][k, :11]], (name, k, dict(zip(pc.STATE, row)))
        for r, c in step["cells"]:
            seen[r, c] = 1
        assert np.array_equal(seen, g["collision"][k]), (name, k)
