"""Goal selection of several episodes in one batched solve (peanut_goal_select_batch / goal.select_batch) against the same
selections made one by one: "alone" is a second set of fresh GeodesicSolvers driven with ``select`` on the same inputs in the same
order, and the gate is equality of bits (stage A is a monotone relaxation, stage B a fixed-point sweep on an acyclic graph: the
field does not depend on the schedule of the rounds -- csrc/goal.hip)."""
import struct
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RES = 5


# ---- seeded map generators: obstacle maps like full_map[0] (fp32, > 0.5 = obstacle) ----
def _maze(h, w, seed, density=0.012):
    rng = np.random.RandomState(seed)
    ob = np.zeros((h, w), np.float32)
    for _ in range(int(density * h * w / 20)):
        r, c = rng.randint(0, h), rng.randint(0, w)
        n = rng.randint(10, 60)
        if rng.rand() < 0.5:
            ob[r:r + 2, c:c + n] = 1
        else:
            ob[r:r + n, c:c + 2] = 1
    ob[rng.randint(0, h, 40), rng.randint(0, w, 40)] = 1
    return ob


def _room(h, w, seed):
    rng = np.random.RandomState(seed)
    ob = np.zeros((h, w), np.float32)
    ob[:3] = ob[-3:] = 1
    ob[:, :3] = ob[:, -3:] = 1
    for _ in range(6):
        r, c = rng.randint(20, h - 30), rng.randint(20, w - 30)
        ob[r:r + 8, c:c + 8] = 1
    return ob


def _corridor(h, w, seed, lane=120):
    """Walls across the map every `lane` rows with a gap at alternating ends: the reachable region is one long corridor."""
    rng = np.random.RandomState(seed)
    ob = np.zeros((h, w), np.float32)
    for k, r in enumerate(range(lane, h - 10, lane)):
        ob[r:r + 3] = 1
        gap = 30 + rng.randint(0, 10)
        if k % 2:
            ob[r:r + 3, :gap] = 0
        else:
            ob[r:r + 3, w - gap:] = 0
    return ob


def _free_around(ob, cell, rad=6):
    ob[max(cell[0] - rad, 0):cell[0] + rad + 1, max(cell[1] - rad, 0):cell[1] + rad + 1] = 0


def _wall_in(ob, cell, rad=3):
    ob[max(cell[0] - rad, 0):cell[0] + rad + 1, max(cell[1] - rad, 0):cell[1] + rad + 1] = 1


def _case(kind, h, w, seed, lmb, loc):
    """One episode's inputs: (obstacles, collision map, visited map, lmb, loc) on the device; `loc` in window coordinates."""
    cell = (lmb[0] + loc[0], lmb[2] + loc[1])
    ob = {"maze": _maze, "room": _room, "corridor": _corridor, "walled": _room}[kind](h, w, seed)
    if kind == "walled":
        _wall_in(ob, cell)
    else:
        _free_around(ob, cell)
    rng = np.random.RandomState(seed + 1000)
    col = np.zeros((h, w), np.uint8)
    col[rng.randint(0, h, 30), rng.randint(0, w, 30)] = 1
    col[cell] = 0
    vis = np.zeros((h, w), np.uint8)
    r = rng.randint(10, h - 40)
    vis[r, 10:w // 3] = 1                                # a visited trail re-opens cells
    return (torch.from_numpy(ob).cuda(), torch.from_numpy(col).cuda(), torch.from_numpy(vis).cuda(), tuple(lmb), tuple(loc))


def _four_960():
    return [_case("maze", 960, 960, 1, (240, 720, 240, 720), (243, 235)),
            _case("room", 960, 960, 2, (200, 680, 260, 740), (100, 300)),
            _case("corridor", 960, 960, 3, (100, 580, 0, 480), (20, 40)),
            _case("walled", 960, 960, 4, (480, 960, 480, 960), (200, 200))]


def _tps(n, lw, lh, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand((lw, lh), generator=g).cuda() for _ in range(n)]


def _solvers(n, h, w, rad=2):
    from peanut_amd.goal import GeodesicSolver
    return [GeodesicSolver(h, w, rad) for _ in range(n)]


def _bits(x):
    return struct.pack("d", x)


def _teq(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def _alone(sols, items, tps, temperature, **want):
    return [s.select(*it, tp, temperature, RES, **want) for s, it, tp in zip(sols, items, tps)]


def _assert_same(got, ref, what=""):
    assert len(got) == len(ref)
    for e, (g, r) in enumerate(zip(got, ref)):
        tag = f"{what} episode {e}"
        assert g["goal"] == r["goal"], tag
        assert _bits(g["wt_sum"]) == _bits(r["wt_sum"]) and _bits(g["value_max"]) == _bits(r["value_max"]), tag
        assert g["kept_last"] == r["kept_last"], tag
        assert g["passes"] == r["passes"] and g["converged"] == r["converged"], (tag, g["passes"], r["passes"])
        for k in ("dist", "value"):
            assert (k in g) == (k in r), tag
            if k in g:
                assert _teq(g[k], r[k]), f"{tag}: {k} differs in {(g[k] != r[k]).sum().item()} cells"


# ---- 1. batch equals alone ----
@pytest.mark.parametrize("temperature", [500.0, 1.0, -1.0, 0.0])
def test_batch_equals_alone_bit_for_bit(temperature):
    from peanut_amd.goal import select_batch
    items = _four_960()
    tps = [None] * 4 if temperature == 0.0 else _tps(4, 480, 480)
    batch, alone = _solvers(4, 960, 960), _solvers(4, 960, 960)
    for rep in range(2):                                   # the second round runs on warm round hints and with last weights
        got = select_batch(batch, items, tps, temperature, RES, want_dist=True, want_value=True)
        ref = _alone(alone, items, tps, temperature, want_dist=True, want_value=True)
        print(f"T={temperature} rep {rep}: passes {[r['passes'] for r in ref]}, alone rounds {[r['rounds'] for r in ref]}, "
              f"batch rounds {got[0]['rounds']}, goals {[r['goal'] for r in ref]}")
        _assert_same(got, ref, f"T={temperature} rep {rep}")
        # condition on the inputs: the done-masking is exercised only if the episodes end their ordering passes at different times
        assert len({r["passes"] for r in ref}) > 1, [r["passes"] for r in ref]
        assert torch.isinf(ref[3]["dist"]).sum().item() >= 960 * 960 - 1      # the walled-in agent reaches nothing


def test_an_episode_at_the_pass_ceiling_is_reported_for_itself_only():
    """All solvers under fmm_max_passes = 6: an episode that stops at the ceiling while others reach their fixed point reports
    converged == False for itself only, with the field of its alone solve, and the Python mirror warns once for that solver."""
    from peanut_amd import _lib
    from peanut_amd.goal import select_batch
    items = _four_960()
    tps = _tps(4, 480, 480)
    with _lib.default_options(fmm_max_passes=6):
        batch, alone = _solvers(4, 960, 960), _solvers(4, 960, 960)
    with warnings.catch_warnings(record=True):
        warnings.simplefilter("always")
        ref = _alone(alone, items, tps, 500.0, want_dist=True)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = select_batch(batch, items, tps, 500.0, RES, want_dist=True)
        select_batch(batch, items, tps, 500.0, RES)
    print(f"cap 6: passes {[r['passes'] for r in ref]}, converged {[r['converged'] for r in ref]}")
    _assert_same(got, ref, "cap 6")
    flags = [r["converged"] for r in ref]
    assert not all(flags) and any(flags), flags            # condition on the inputs: one at the ceiling, others at their fixed point
    said = [r for r in rec if "ordering passes stopped at their cap" in str(r.message)]
    assert len(said) == flags.count(False), [str(r.message) for r in rec]
    assert [s.converged for s in batch] == flags


# ---- 2. it really is one solve ----
def test_the_batch_enqueues_the_rounds_of_one_solve():
    from peanut_amd.goal import select_batch
    items = _four_960()
    tps = _tps(4, 480, 480)
    got = select_batch(_solvers(4, 960, 960), items, tps, 500.0, RES)
    ref = _alone(_solvers(4, 960, 960), items, tps, 500.0)
    rounds = [r["rounds"] for r in ref]
    print(f"alone rounds {rounds} (sum {sum(rounds)}), batch rounds {got[0]['rounds']}")
    assert len({g["rounds"] for g in got}) == 1
    assert max(rounds) <= got[0]["rounds"] < sum(rounds)


# ---- 3. state carried across a changing batch ----
def test_state_is_carried_across_a_changing_batch():
    from peanut_amd.goal import select_batch, select_begin_batch
    H = W = 480
    lmbs = [(100, 340, 100, 340), (0, 240, 240, 480), (120, 360, 60, 300), (240, 480, 0, 240)]
    locs = [(120, 120), (60, 200), (100, 30), (200, 100)]
    kinds = ["maze", "room", "maze", "corridor"]
    base = [_case(k, H, W, 10 + e, lmbs[e], locs[e]) for e, k in enumerate(kinds)]
    tps = _tps(4, 240, 240, seed=5)
    batch, alone = _solvers(4, H, W), _solvers(4, H, W)
    kept = []

    def items_at(step, which, stuck=(), lmb_of=None):
        out = []
        for e in which:
            ob, col, vis, lmb, loc = base[e]
            ob = ob.clone()
            ob[20 + 7 * step:24 + 7 * step, 30 + 40 * e:90 + 40 * e] = 1.0        # the map changes slowly
            cell = (lmb[0] + loc[0], lmb[2] + loc[1])
            if e in stuck:
                ob[cell[0] - 3:cell[0] + 4, cell[1] - 3:cell[1] + 4] = 1.0        # the agent's cell and its surroundings are blocked
            out.append((ob, col, vis, lmb if lmb_of is None else lmb_of[e], loc))
        return out

    def step(n, which, begin=False, single=False, **kw):
        its = items_at(n, which, **kw)
        lw, lh = its[0][3][1] - its[0][3][0], its[0][3][3] - its[0][3][2]
        tp = [tps[e][:lw, :lh].contiguous() for e in which]
        if single:
            got = [batch[which[0]].select(*its[0], tp[0], 500.0, RES, want_dist=True, want_value=True)]
        else:
            if begin:
                select_begin_batch([batch[e] for e in which], its)
            got = select_batch([batch[e] for e in which], its, tp, 500.0, RES, want_dist=True, want_value=True)
        ref = _alone([alone[e] for e in which], its, tp, 500.0, want_dist=True, want_value=True)
        _assert_same(got, ref, f"step {n}")
        kept.append([r["kept_last"] for r in ref])
        return ref

    step(0, [0, 1, 2, 3])
    step(1, [0, 2])
    step(2, [1], single=True)
    step(3, [0, 1, 2, 3])
    n0 = [batch[e].begun_matches for e in (1, 3)]
    step(4, [1, 3], begin=True)
    assert [batch[e].begun_matches for e in (1, 3)] == [n + 1 for n in n0]
    ref = step(5, [0, 1, 2, 3], stuck=(2,))
    assert ref[2]["kept_last"] and ref[2]["wt_sum"] < 10 and [r["kept_last"] for r in ref] == [False, False, True, False]
    # a window of another size, for ALL episodes: the last weights are forgotten, as the single call forgets them
    small = [(l[0], l[0] + 200, l[2], l[2] + 200) for l in lmbs]
    ref = step(6, [0, 1, 2, 3], stuck=(2,), lmb_of=small)
    assert not any(r["kept_last"] for r in ref)
    assert any(any(k) for k in kept)


# ---- 4. begin ----
def test_begun_batch_is_taken_over_and_anything_else_solves_alone():
    from peanut_amd.goal import select_batch, select_begin_batch
    items = _four_960()
    tps = _tps(4, 480, 480)
    batch, alone = _solvers(4, 960, 960), _solvers(4, 960, 960)
    ref = _alone(alone, items, tps, 500.0, want_dist=True, want_value=True)
    a = torch.randn((2048, 2048), device="cuda")
    select_begin_batch(batch, items)
    for _ in range(6):                                      # a chain of large products on the caller's stream, beside the fields
        a = torch.tanh(a @ a * 1e-3)
    got = select_batch(batch, items, tps, 500.0, RES, want_dist=True, want_value=True)
    assert [s.begun_matches for s in batch] == [1] * 4
    _assert_same(got, ref, "begun")
    # another agent cell for one episode: the begun fields run out, these inputs are solved
    moved = list(items)
    moved[1] = moved[1][:4] + ((140, 260),)
    _free = moved[1][0]
    ref2 = _alone(alone, moved, tps, 500.0, want_dist=True, want_value=True)
    select_begin_batch(batch, items)
    got = select_batch(batch, moved, tps, 500.0, RES, want_dist=True, want_value=True)
    _assert_same(got, ref2, "moved")
    assert not _teq(ref2[1]["dist"], ref[1]["dist"]) and _free is items[1][0]
    # a single select on one of the begun handles; then the whole batch again
    select_begin_batch(batch, items)
    one = batch[2].select(*items[2], tps[2], 500.0, RES, want_dist=True, want_value=True)
    _assert_same([one], [alone[2].select(*items[2], tps[2], 500.0, RES, want_dist=True, want_value=True)], "single after begin")
    got = select_batch(batch, items, tps, 500.0, RES, want_dist=True, want_value=True)
    _assert_same(got, _alone(alone, items, tps, 500.0, want_dist=True, want_value=True), "batch after single")
    # distance() on a begun handle
    trav = batch[0].traversible(items[0][0], items[0][1], items[0][2])
    cell = (items[0][3][0] + items[0][4][0], items[0][3][2] + items[0][4][1])
    select_begin_batch(batch, items)
    d = batch[0].distance(trav, goal=cell)
    assert _teq(d, alone[0].distance(trav, goal=cell))
    got = select_batch(batch, items, tps, 500.0, RES, want_dist=True, want_value=True)
    _assert_same(got, _alone(alone, items, tps, 500.0, want_dist=True, want_value=True), "batch after distance")


def test_begin_batch_on_reused_storage_or_edited_inputs_solves_the_new_inputs():
    """The cases of test_select_begin_on_reused_storage_or_edited_inputs_solves_the_new_inputs for a batch of two."""
    from peanut_amd.goal import select_batch, select_begin_batch
    H = W = 240
    lmb, locs = (40, 200, 40, 200), [(80, 80), (60, 100)]
    obs = []
    for e in range(2):
        ob = _maze(H, W, 31 + e)
        _free_around(ob, (40 + locs[e][0], 40 + locs[e][1]), 10)
        obs.append(torch.from_numpy(ob).cuda())
    col_a = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    col_b = col_a.clone()
    col_b[40 + 50:40 + 110, 40 + 90] = 1                 # a wall next to the agents: other fields
    vis = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    tps = _tps(2, 160, 160, seed=3)
    batch, alone = _solvers(2, H, W, 1), _solvers(2, H, W, 1)

    def begin_on_temporaries():
        ts = [col_a.bool(), col_a.bool()]
        select_begin_batch(batch, [(obs[e], ts[e], vis, lmb, locs[e]) for e in range(2)])
        return [t.data_ptr() for t in ts]

    ptrs = begin_on_temporaries()
    tb = [col_b.bool(), col_b.bool()]
    print(f"allocator handed the begun temporaries' blocks to the next ones: {[t.data_ptr() in ptrs for t in tb]}")
    its = [(obs[e], tb[e], vis, lmb, locs[e]) for e in range(2)]
    got = select_batch(batch, its, tps, 500.0, RES, want_dist=True, want_value=True)
    _assert_same(got, _alone(alone, its, tps, 500.0, want_dist=True, want_value=True), "temporaries")
    # written in place between begin and select
    ob2 = [o.clone() for o in obs]
    its = [(ob2[e], col_a, vis, lmb, locs[e]) for e in range(2)]
    select_begin_batch(batch, its)
    ob2[1][40 + 40:40 + 120, 40 + 85] = 1.0
    got = select_batch(batch, its, tps, 500.0, RES, want_dist=True, want_value=True)
    _assert_same(got, _alone(alone, its, tps, 500.0, want_dist=True, want_value=True), "edited in place")
    # ... through views of larger maps (Agent_State passes full_map[0])
    full = [torch.stack([o, o * 0]) for o in obs]
    its = [(full[e][0], col_a, vis, lmb, locs[e]) for e in range(2)]
    select_begin_batch(batch, its)
    full[0][0, 40 + 75, 40 + 40:40 + 120] = 1.0
    its = [(full[e][0], col_a, vis, lmb, locs[e]) for e in range(2)]
    got = select_batch(batch, its, tps, 500.0, RES, want_dist=True, want_value=True)
    ref = _alone(alone, its, tps, 500.0, want_dist=True, want_value=True)
    _assert_same(got, ref, "edited view")
    n0 = [s.begun_matches for s in batch]
    select_begin_batch(batch, its)                          # unchanged inputs: the begun fields are taken over
    got = select_batch(batch, [(full[e][0], col_a, vis, lmb, locs[e]) for e in range(2)], tps, 500.0, RES, want_dist=True)
    assert [s.begun_matches for s in batch] == [n + 1 for n in n0]
    assert all(_teq(g["dist"], r["dist"]) for g, r in zip(got, ref))


# ---- 5. refusals ----
def test_refusals_raise_and_leave_the_solvers_usable():
    from peanut_amd.goal import GeodesicSolver, select_batch, select_begin_batch
    H = W = 240
    lmb = (40, 200, 40, 200)
    items = [_case("maze", H, W, 40 + e, lmb, (80, 70 + 5 * e)) for e in range(3)]
    tps = _tps(3, 160, 160)
    batch, alone = _solvers(3, H, W, 1), _solvers(3, H, W, 1)
    other_size, other_rad = GeodesicSolver(200, 240, 1), GeodesicSolver(H, W, 2)
    many = _solvers(17, 64, 64, 1)
    small = [_case("room", 64, 64, 1, (0, 32, 0, 32), (10, 10))] * 17
    bad = [
        lambda: select_batch([], [], [], 500.0, RES),
        lambda: select_batch(many, small, _tps(17, 32, 32), 500.0, RES),
        lambda: select_begin_batch(many, small),
        lambda: select_batch([batch[0], batch[1], batch[0]], items, tps, 500.0, RES),
        lambda: select_batch([batch[0], other_size], items[:2], tps[:2], 500.0, RES),
        lambda: select_batch([batch[0], other_rad], items[:2], tps[:2], 500.0, RES),
        lambda: select_begin_batch([batch[0], other_rad], items[:2]),
        lambda: select_batch(batch[:2], [items[0], items[1][:3] + ((40, 180, 40, 200), items[1][4])], tps[:2], 500.0, RES),
        lambda: select_batch(batch[:2], items[:2], [tps[0], tps[1][:100]], 500.0, RES),
        lambda: select_batch(batch[:2], items[:2], None, 500.0, RES),
        lambda: select_batch(batch[:2], [items[0], items[1][:3] + ((100, 260, 40, 200), items[1][4])], tps[:2], 500.0, RES),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(Exception) as err:
            call()
        assert isinstance(err.value, (ValueError, RuntimeError)), (k, err.value)
        got = select_batch(batch, items, tps, 500.0, RES, want_dist=True, want_value=True)
        _assert_same(got, _alone(alone, items, tps, 500.0, want_dist=True, want_value=True), f"after refusal {k}")


# ---- 6. the ends of the range ----
def test_one_episode_equals_select_and_sixteen_equal_alone():
    from peanut_amd.goal import select_batch
    it = _four_960()[0]
    tp = _tps(1, 480, 480)
    got = select_batch(_solvers(1, 960, 960), [it], tp, 500.0, RES, want_dist=True, want_value=True)
    ref = _alone(_solvers(1, 960, 960), [it], tp, 500.0, want_dist=True, want_value=True)
    _assert_same(got, ref, "E = 1")
    assert got[0]["rounds"] == ref[0]["rounds"]
    H = W = 480
    kinds = ["maze", "room", "corridor", "walled"]
    items = [_case(kinds[e % 4], H, W, 60 + e, (10 * e, 10 * e + 240, 240 - 10 * e, 480 - 10 * e), (30 + 10 * e, 200 - 8 * e)) for e in range(16)]
    tps = _tps(16, 240, 240, seed=7)
    batch, alone = _solvers(16, H, W), _solvers(16, H, W)
    for rep in range(2):
        got = select_batch(batch, items, tps, 500.0, RES, want_dist=True, want_value=True)
        _assert_same(got, _alone(alone, items, tps, 500.0, want_dist=True, want_value=True), f"E = 16 rep {rep}")


def test_ragged_tiles():
    from peanut_amd.goal import select_batch
    H, W = 250, 333
    items = [_case(k, H, W, 80 + e, (5 + 3 * e, 205 + 3 * e, 20 + e, 320 + e), (100 + e, 150 - 7 * e)) for e, k in enumerate(["maze", "room", "walled"])]
    tps = _tps(3, 200, 300, seed=9)
    got = select_batch(_solvers(3, H, W, 3), items, tps, 500.0, RES, want_dist=True, want_value=True)
    _assert_same(got, _alone(_solvers(3, H, W, 3), items, tps, 500.0, want_dist=True, want_value=True), "250 x 333")


# ---- 7. the agent's own pair, real model ----
@pytest.mark.parametrize("precision", ["fp32", "fp16x3"])
def test_lockstep_episodes_with_batched_goals_equal_those_without(precision, monkeypatch):
    from oracle import mapping_scenes
    from oracle.agent_ref import agent_args
    from peanut_amd import goal as G
    from peanut_amd.agent_state import Agent_State
    from peanut_amd.prediction import PEANUT_Prediction_Model
    from peanut_amd.replay import run_episodes
    from peanut_amd.weights import PredCfg, make_seeded_state_dict
    args = agent_args(dist_weight_temperature=500, select_goal=True, goal_overlap=True, pred_precision=precision, only_explore=0)
    model = PEANUT_Prediction_Model(args, state_dict=make_seeded_state_dict(PredCfg(), 0))
    seeds, cats = (11, 12, 13), (2, 1, 4)
    eps = []
    for seed in seeds:
        frames = mapping_scenes.make_sequence(seed=seed, n_frames=24)
        eps.append([dict(obs=torch.from_numpy(mapping_scenes.frame_to_obs(fr))[None].cuda(), sensor_pose=[float(v) for v in fr["pose"]])
                    for fr in frames])
    calls = []
    real = G.select_batch
    monkeypatch.setattr(G, "select_batch", lambda solvers, *a, **k: (calls.append(len(list(solvers))), real(solvers, *a, **k))[1])
    runs = []
    for batched in (True, False):
        states = [Agent_State(args, prediction_model=model) for _ in seeds]
        rec, due = [], []

        def on_step(i, act, predicted, rec=rec, due=due):
            due.append(sum(predicted))
            for s, p in zip(act, predicted):
                if p:
                    rec.append((i, tuple(s.global_goals[0]), s.target_pred.clone(), _bits(s.value_max)))
        del calls[:]
        n_pred = run_episodes(states, eps, cats, on_step=on_step, batch_goals=batched)
        runs.append((n_pred, rec, [s.full_map.clone() for s in states], list(calls), due, [s._goal.begun_matches for s in states]))
    (n_a, rec_a, maps_a, calls_a, due_a, begun_a), (n_b, rec_b, maps_b, calls_b, _, _) = runs
    assert n_a == n_b and min(n_a) >= 2 and len(rec_a) == len(rec_b)
    for x, y in zip(rec_a, rec_b):
        assert x[0] == y[0] and x[1] == y[1] and x[3] == y[3] and torch.equal(x[2], y[2]), (x[0], x[1], y[1])
    assert all(torch.equal(a, b) for a, b in zip(maps_a, maps_b))
    # every predicting step with >= 2 due episodes went through select_batch, over all of them, and took over its begun fields
    assert calls_a == [d for d in due_a if d >= 2] and len(calls_a) >= 2 and calls_b == []
    assert begun_a == n_a


# ---- 8. the other kernels of the round: options fmm_blocked, fmm_local32, fmm_inner ----
@pytest.mark.parametrize("blocked,local32,inner", [(1, 1, 1), (1, 1, 1024), (1, 0, 48), (1, 0, 1), (1, 0, 1024), (0, 1, 48), (0, 0, 48)], ids=lambda v: str(v))
def test_solver_variants_batched_equal_alone_bit_for_bit(blocked, local32, inner):
    """enqueue_rounds_batch (csrc/goal.hip) picks one of four batch kernels as the single solve does -- fmm_round_blocked_batch_kernel
    or fmm_round_batch_kernel, with the single-precision or the float64 local solve -- and only (blocked, local32) = (1, 1) with 48
    inner iterations runs above.  Three ragged 250 x 333 episodes (a maze, a room, a walled-in agent) under every other setting:
    the batch equals the three alone solves on solvers of the same setting bit for bit, twice (the second time on warm round hints
    and last weights).  That the setting reached the kernels shows against a default solver on the same episodes: the float64
    local solve, the whole-tile sweep and fmm_inner = 1 give other bits in the maze's field (another schedule lands elsewhere inside
    stage B's noise threshold); fmm_inner = 1024 only reschedules (a block has converged long before), so there the field equals the
    default's bit for bit.  The variants pick the default's goals."""
    from peanut_amd import _lib
    from peanut_amd.goal import select_batch
    H, W = 250, 333
    items = [_case(k, H, W, 80 + e, (5 + 3 * e, 205 + 3 * e, 20 + e, 320 + e), (100 + e, 150 - 7 * e)) for e, k in enumerate(["maze", "room", "walled"])]
    tps = _tps(3, 200, 300, seed=9)
    with _lib.default_options(fmm_blocked=blocked, fmm_local32=local32, fmm_inner=inner):
        batch, alone = _solvers(3, H, W, 3), _solvers(3, H, W, 3)
    for rep in range(2):
        got = select_batch(batch, items, tps, 500.0, RES, want_dist=True, want_value=True)
        ref = _alone(alone, items, tps, 500.0, want_dist=True, want_value=True)
        _assert_same(got, ref, f"blocked={blocked} local32={local32} inner={inner} rep {rep}")
    assert torch.isinf(ref[2]["dist"]).sum().item() >= H * W - 1          # the walled-in agent reaches nothing
    base = _alone(_solvers(3, H, W, 3), items, tps, 500.0, want_dist=True, want_value=True)
    differs = int((ref[0]["dist"] != base[0]["dist"]).sum().item())
    print(f"blocked={blocked} local32={local32} inner={inner}: rounds alone {[r['rounds'] for r in ref]} batch {got[0]['rounds']}, default "
          f"{[r['rounds'] for r in base]}; {differs} cells of the maze's field differ from the default's in some bit")
    assert [r["goal"] for r in ref] == [r["goal"] for r in base]
    assert torch.equal(torch.isfinite(ref[0]["dist"]), torch.isfinite(base[0]["dist"]))
    if not local32 or not blocked or inner == 1:
        assert differs > 0, "the default kernels' field, bit for bit"
    else:
        assert differs == 0
