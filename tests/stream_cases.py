"""The ordering contract of include/peanut_hip.h ("functions enqueue on the given hipStream_t ... and do not synchronise unless
stated") as test infrastructure, importable without a GPU: tests/test_streams_cpu.py checks the tables, tests/test_streams_gpu.py
runs the protocols.

``CONTRACT``      one row per prototype that takes a ``void* stream``: "async" (the header promises no synchronisation), "syncs" (the
                  header says the call synchronises the caller's stream) or "exempt" (with a reason).  Classed from the header's words.
``backlog()``     a bounded delay on a stream (``torch.cuda._sleep``: one spinning thread, every CU stays free for work that wrongly
                  runs early) and an event recorded right behind it.  The delay always ends by itself; nothing here waits for a
                  condition that a bug could keep from coming true.
``p1 / p2 / p3``  the three protocols, generic over ``make() -> handle`` and ``run(handle, inputs, outs) -> result``; results are
                  compared with ``workspace_cases.same`` (bit equality) against the same call on an idle default stream.
``INPUTS``        per case name the deterministic builder ``seed -> tuple of CPU tensors`` of the call's input buffers: seed 0 is
                  ``x_good``, seed 1 ``x_stale`` (same shapes, same value range: valid data), seeds 2.. the further inputs of p2 / p3.
"""
import os
import time

import numpy as np
import torch

from workspace_cases import first_difference, same

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

# ---------------------------------------------------------------------------------------------------------------------------------
# the contract
# ---------------------------------------------------------------------------------------------------------------------------------
_ASYNC = """peanut_conv_forward peanut_pred_forward peanut_pred_debug_read
peanut_map_forward peanut_map_forward_batch peanut_map_mark_agent peanut_map_mark_agent_batch
peanut_goal_map peanut_goal_map_batch
peanut_rcnn_forward_front peanut_rcnn_preprocess
peanut_roi_align peanut_nms peanut_nms_segments peanut_paste_masks
peanut_preprocess_obs peanut_preprocess_obs_batch peanut_seg_accumulate
peanut_goal_traversible peanut_goal_select_begin peanut_goal_select_begin_batch
peanut_stg_traversible peanut_stg_goal peanut_stg_window""".split()
_SYNCS = """peanut_fmm_distance peanut_goal_select peanut_goal_select_batch
peanut_rcnn_inference peanut_rcnn_semantic peanut_stg_plan""".split()
_EXEMPT = {
    "peanut_allgather_maps": "a collective of several processes: ordering is held by tests/test_dist_gpu.py",
    "peanut_debug_lds_canary": "a debug canary that exists to run BESIDE another stream's kernel, not behind it",
    "peanut_debug_pkfma_canary": "a debug canary that exists to run BESIDE another stream's kernel, not behind it",
    "peanut_rcnn_probe_front": "an event probe: it times the front end and synchronises by design; it returns timings, no tensors",
}
CONTRACT = {**{s: ("async", "") for s in _ASYNC}, **{s: ("syncs", "") for s in _SYNCS}, **{s: ("exempt", r) for s, r in _EXEMPT.items()}}


def klass(symbol):
    return CONTRACT[symbol][0]


# ---------------------------------------------------------------------------------------------------------------------------------
# the backlog
# ---------------------------------------------------------------------------------------------------------------------------------
NOMINAL_MS = 50.0
CAP_MS = 200.0
_CALIBRATION_CYCLES = 2_000_000
_delay = {}          # "method": "sleep" | "mm"; "per_ms": cycles (sleep) or matrix products (mm) per millisecond


def _elapsed_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def calibrate():
    """Once per process: cycles of ``torch.cuda._sleep`` per millisecond, from two timing events around a fixed sleep (as torch's own
    test utilities do); a chain of 2048^3 matrix products timed the same way where ``_sleep`` is missing or does not delay."""
    if _delay:
        return _delay
    sleep = getattr(torch.cuda, "_sleep", None)
    if sleep is not None:
        sleep(_CALIBRATION_CYCLES)                                   # (first use: loads the kernel)
        ms = _elapsed_ms(lambda: sleep(_CALIBRATION_CYCLES))
        if ms >= 0.2:
            _delay.update(method="sleep", per_ms=_CALIBRATION_CYCLES / ms)
    if not _delay:
        a = torch.ones((2048, 2048), device="cuda")
        torch.mm(a, a)
        ms = _elapsed_ms(lambda: [torch.mm(a, a) for _ in range(16)])
        _delay.update(method="mm", per_ms=16.0 / ms, operand=a)
    print(f"stream backlog: method {_delay['method']}, {_delay['per_ms']:.1f} per ms")
    return _delay


def backlog(stream, ms=NOMINAL_MS):
    """Enqueue a delay of ``ms`` (at most CAP_MS) on ``stream`` -> the ``torch.cuda.Event`` recorded right behind it."""
    d = calibrate()
    ms = min(float(ms), CAP_MS)
    with torch.cuda.stream(stream):
        if d["method"] == "sleep":
            torch.cuda._sleep(int(ms * d["per_ms"]))
        else:
            for _ in range(max(1, int(round(ms * d["per_ms"])))):
                torch.mm(d["operand"], d["operand"])
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev


# ---------------------------------------------------------------------------------------------------------------------------------
# the protocols
# ---------------------------------------------------------------------------------------------------------------------------------
def snapshot(tree):
    """A copy of a result that no later call can touch."""
    if isinstance(tree, torch.Tensor):
        return tree.clone()
    if isinstance(tree, dict):
        return {k: snapshot(v) for k, v in tree.items()}
    if isinstance(tree, (list, tuple)):
        return type(tree)(snapshot(v) for v in tree)
    return tree


def assert_same(got, want, what):
    assert same(got, want), f"{what}: {first_difference(got, want)}"


def _sentinel(outs):
    for t in outs or ():
        t.view(torch.uint8).fill_(0xA5)


def to_device(xs):
    return [t.cuda() for t in xs]


def p1(name, make, run, good, stale, cls, outs=None, ms=NOMINAL_MS, reps=1, warm=True, after=None):
    """Late input, early overwrite.  ``good`` / ``stale``: lists of device tensors.  Plainly (default stream, full synchronisation)
    ``r_good = run(h, good)`` and ``r_stale = run(h, stale)`` must differ.  Then on a fresh side stream, ``reps`` times and with no host
    synchronisation between the four steps: a backlog; the input buffers (holding ``stale``) are overwritten with ``good``; the call;
    the buffers are overwritten with ``stale`` again.  After ``side.synchronize()`` the result is ``r_good`` bit for bit.  For an
    "async" row the backlog's event must still be pending when the call returns -- asserted on a steady-state call: after one warm-up
    call on the side stream (``warm``), or else on the last repetition (graph modes: direct, captured, replayed).
    ``after(handle)``: a host-side check once everything is synchronised (kernel family, counters)."""
    h = make()
    _sentinel(outs)
    r_good = snapshot(run(h, good, outs))
    torch.cuda.synchronize()
    _sentinel(outs)
    r_stale = snapshot(run(h, stale, outs))
    torch.cuda.synchronize()
    assert not same(r_good, r_stale), f"{name}: the two inputs give one result; the case cannot tell a stale read"
    x = [t.clone() for t in stale]
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    pending = None
    with torch.cuda.stream(side):
        if warm:
            run(h, x, outs)
            side.synchronize()
        for rep in range(reps):
            _sentinel(outs)
            ev = backlog(side, ms)
            for xi, g in zip(x, good):
                xi.copy_(g, non_blocking=True)
            t0 = time.perf_counter()
            res = run(h, x, outs)
            host_ms = (time.perf_counter() - t0) * 1e3
            pending = not ev.query()
            for xi, s in zip(x, stale):
                xi.copy_(s, non_blocking=True)
            side.synchronize()
            assert_same(snapshot(res), r_good, f"{name}: behind a {ms:.0f} ms backlog, call {rep}")
            assert all(same(xi, s) for xi, s in zip(x, stale))
    torch.cuda.synchronize()
    # (with `pytest -s` these lines are the table of enqueue times in DESIGN.md sec. 10)
    print(f"HOSTMS {name} {cls} {host_ms:.3f} ms, backlog pending at return: {pending}")
    if cls == "async":
        assert pending, f"{name}: the call returned only after the {ms:.0f} ms backlog had drained: it synchronises"
    if after is not None:
        after(h)
    return h


def p2(name, make, run, xs, ms=NOMINAL_MS, after=None, plain_make=None):
    """Back to back.  ``xs``: three (or more) input lists, the second of another and larger shape.  Plain results come from one handle
    on the default stream with full synchronisation; then a FRESH handle (it has seen none of the shapes: plans, scratch and cached
    graphs are made and regrown under in-flight work) runs all calls behind one backlog with no host synchronisation, and each output
    equals its own plain result.  ``plain_make``: another factory for the handle of the plain results (one the module keeps)."""
    h = (plain_make or make)()
    plain = []
    for x in xs:
        plain.append(snapshot(run(h, x, None)))
        torch.cuda.synchronize()
    assert not same(plain[0], plain[-1]), f"{name}: the first and the last call give one result"
    h2 = make()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        backlog(side, ms)
        res = [run(h2, x, None) for x in xs]
        side.synchronize()
    for k, (r, want) in enumerate(zip(res, plain)):
        assert_same(r, want, f"{name}: back-to-back call {k}")
    torch.cuda.synchronize()
    if after is not None:
        after(h2)
    return h2


def p3(name, makes, runs, xs, rounds=2, ms=NOMINAL_MS):
    """Two handles, two streams: each handle on its own side stream behind its own backlog, calls enqueued alternately; every result
    equals the one the same handle gave alone (default stream, full synchronisation, the other handle idle)."""
    handles = [make() for make in makes]
    alone = []
    for h, run, x in zip(handles, runs, xs):
        alone.append(snapshot(run(h, x, None)))
        torch.cuda.synchronize()
    sides = [torch.cuda.Stream() for _ in makes]
    torch.cuda.synchronize()
    for s in sides:
        backlog(s, ms)
    res = [[] for _ in makes]
    for _ in range(rounds):
        for i, (h, run, x, s) in enumerate(zip(handles, runs, xs, sides)):
            with torch.cuda.stream(s):
                res[i].append(run(h, x, None))
    for s in sides:
        s.synchronize()
    for i, want in enumerate(alone):
        for k, r in enumerate(res[i]):
            assert_same(r, want, f"{name}: handle {i}, call {k}")
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs (CPU tensors; seed 0 = good, 1 = stale, 2.. = further calls)
# ---------------------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(7919 * seed + 11)


def randn(shapes):
    return lambda seed: tuple(torch.randn(s, generator=_gen(seed)) for s in shapes)


def binary_maps(shape):
    """Prediction inputs, the recipe of tests/test_pred_gpu.py (_inputs): a binary map per channel."""
    return lambda seed: ((torch.rand(shape, generator=_gen(seed)) > 0.7).float(),)


def golden_pred_input(name):
    """seed 0: the committed golden input ``name`` of pspnet_golden.npz; other seeds: binary maps of its shape."""
    def build(seed):
        z = np.load(os.path.join(GOLDEN, "pspnet_golden.npz"))
        x = torch.from_numpy(z[f"{name}/input"].astype(np.float32))
        return (x,) if seed == 0 else binary_maps(tuple(x.shape))(seed)
    return build


def frames(shape=(2, 96, 128, 3)):
    return lambda seed: (torch.randint(0, 256, shape, generator=_gen(seed), dtype=torch.uint8),)


def map_frames(E=1, with_maps=True):
    """(obs [E,14,120,160], pose_obs [E,3], maps_last [E,14,480,480]) from the golden sequences: episode e of seed s reads frame
    (s + e) % 5 of seq0 (even s + e) or seq1 (odd); maps_last is a sparse non-negative map."""
    def build(seed):
        z = np.load(os.path.join(GOLDEN, "mapping_golden.npz"))
        obs = np.zeros((E, 14, 120, 160), np.float32)
        rel = np.zeros((E, 3), np.float32)
        for e in range(E):
            k = seed + e
            name, i = ("seq0", "seq1")[k % 2], k % 5
            obs[e, 3] = z[f"{name}/depth"][i]
            obs[e, 4:] = z[f"{name}/sem"][i].astype(np.float32)
            rel[e] = z[f"{name}/pose_obs"][i]
        g = _gen(seed)
        maps = (torch.rand((E, 14, 480, 480), generator=g) > 0.98).float() * torch.rand((E, 14, 480, 480), generator=g)
        out = (torch.from_numpy(obs), torch.from_numpy(rel))
        return out + (maps,) if with_maps else out
    return build


def raw_obs(E=1, H=480, W=640, ncat=10):
    """(rgb u8, depth in [0, 1.1) with invalid pixels and columns, sem 0 / 1): the recipe of test_preprocess_obs_matches_reference_loop."""
    def build(seed):
        rng = np.random.RandomState(100 + seed)
        depth = rng.uniform(0.0, 1.1, size=(E, H, W)).astype(np.float32)
        depth[rng.uniform(size=(E, H, W)) < 0.1] = 0.0
        depth[:, :, 100:140] = 0.0
        rgb = rng.randint(0, 256, size=(E, H, W, 3)).astype(np.uint8)
        sem = (rng.uniform(size=(E, H, W, ncat)) > 0.9).astype(np.float32)
        if E == 1:
            rgb, depth, sem = rgb[0], depth[0], sem[0]
        return torch.from_numpy(rgb), torch.from_numpy(depth), torch.from_numpy(sem)
    return build


def goal_maps(h, w, lmb, E=1):
    """(obstacles [h,w] f32, collision u8, target_pred) per episode: _goal_inputs of tests/test_workspace_gpu.py."""
    def build(seed):
        import test_goal_gpu as tg
        out = []
        for e in range(E):
            s = 4 + 3 * seed + e
            col = torch.zeros((h, w), dtype=torch.uint8)
            col[h // 2 + seed, w // 4:w // 2] = 1
            tp = torch.rand((lmb[1] - lmb[0], lmb[3] - lmb[2]), generator=torch.Generator().manual_seed(s))
            out += [tg._obstacles(h, w, s), col, tp]
        return tuple(out)
    return build


def goal_map_parents(E=1):
    """Per episode a [14, 2m, 2m] parent holding a random case of tests/goal_map_cases.py at rows 7.., columns m - 3..: the call
    reads the strided view."""
    def build(seed):
        import goal_map_cases as gmc
        cases = gmc.random_cases()
        out = []
        for e in range(E):
            lm = cases[(2 * seed + 2 * e) % len(cases)]["local_map"]         # even cases: a blob that survives the erosions
            m = lm.shape[1]
            parent = torch.rand((gmc.C, 2 * m, 2 * m), generator=_gen(seed + e)) * 0.5 + 0.25
            parent[:, 7:7 + m, m - 3:2 * m - 3] = torch.from_numpy(lm)
            out.append(parent)
        return tuple(out)
    return build


def stg_masks(seed):
    """(obstacle, goal, collision, visited) of two mask cases of tests/stg_cases.py with one map size (m = 61)."""
    import stg_cases
    c = stg_cases.mask_cases()[(0, 3, 6, 9)[seed % 4]]
    assert c["m"] == 61
    return tuple(torch.from_numpy(c[k]) for k in ("obstacle", "goal", "collision", "visited"))


def stg_fields(seed):
    import stg_cases
    f = stg_cases.window_fields()
    return (torch.from_numpy(f[("euclid", "manhattan", "plateau")[seed % 3]]),)


def stg_scenes(seed):
    """The maps of the m = 61 scenes: blocked_start (the retry scene: good), doors, and blocked_start with its goal four cells nearer."""
    import stg_cases
    by = {c["name"]: c for c in stg_cases.scene_cases()}
    c = dict(by[("blocked_start", "doors", "blocked_start")[seed % 3]])
    if seed % 3 == 2:
        c["goal"] = c["goal"].copy()
        c["goal"][12, 50], c["goal"][12, 46] = 0, 1
    return tuple(torch.from_numpy(c[k]) for k in ("obstacle", "goal", "collision", "visited"))


def roi_inputs(seed):
    """test_roi_align_matches_restatement's recipe, NHWC: four levels [2, 64 >> l, 80 >> l, 32], 50 rois over all levels."""
    g = _gen(seed)
    pyr = [torch.randn((2, 64 >> l, 80 >> l, 32), generator=g) for l in range(4)]
    gr = torch.Generator().manual_seed(3)                           # the boxes (hence the levels) are the same for every seed
    xy = torch.rand((50, 2), generator=gr) * torch.tensor([250.0, 200.0])
    wh = torch.exp(torch.rand((50, 2), generator=gr) * 6.0)
    rois = torch.cat([torch.randint(0, 2, (50, 1), generator=gr).float(), xy, xy + wh], 1)
    rois[0, 1:] = torch.tensor([-20.0, -10.0, 30.0, 500.0])        # sticks out of the map on every side
    rois[2, 1:] = torch.tensor([5.0, 3.0, 610.0, 480.0])           # sqrt(area) >= 448 -> p5
    return tuple(pyr) + (rois,)


def nms_boxes(counts=(130, 0, 70, 257)):
    def build(seed):
        g = _gen(seed)
        n = sum(counts)
        ctr, size = torch.rand((n, 2), generator=g) * 100.0, torch.rand((n, 2), generator=g) * 30.0 + 10.0
        return torch.cat([ctr - size / 2, ctr + size / 2], 1), torch.randint(0, 3, (n,), generator=g, dtype=torch.int32)
    return build


def paste_inputs(seed):
    g = _gen(seed)
    n, M = 9, 28
    probs = torch.rand((n, M, M), generator=g)
    xy = torch.rand((n, 2), generator=g) * torch.tensor([60.0, 40.0])
    return probs, torch.cat([xy, xy + torch.rand((n, 2), generator=g) * 40 + 0.5], 1)


def seg_inputs(seed):
    g = _gen(seed)
    n, H, W = 5, 120, 160
    masks = (torch.rand((n, H, W), generator=g) > 0.6).to(torch.uint8)
    return masks, torch.randint(0, 9, (n,), generator=g, dtype=torch.int32), torch.rand((n,), generator=g) * 0.5 + 0.5


GOAL_SMALL = dict(shape=(64, 40), lmb=(8, 56, 4, 36), loc=(20, 15))
GOAL_BIG = dict(shape=(250, 333), lmb=(20, 220, 40, 300), loc=(100, 130))

INPUTS = {
    "pred_rect": golden_pred_input("rect_72x104"),
    "pred_96": binary_maps((1, 14, 96, 96)),
    "pred_big": binary_maps((1, 14, 200, 200)),
    "det_frames": frames((2, 96, 128, 3)),
    "det_frame1": frames((1, 96, 128, 3)),
    "map_single": map_frames(1),
    "map_batch4": map_frames(4),
    "obs_single": raw_obs(1),
    "obs_batch3": raw_obs(3),
    "goal_small": goal_maps(*GOAL_SMALL["shape"], GOAL_SMALL["lmb"]),
    "goal_big": goal_maps(*GOAL_BIG["shape"], GOAL_BIG["lmb"]),
    "goal_big3": goal_maps(*GOAL_BIG["shape"], GOAL_BIG["lmb"], E=3),
    "goal_map_view": goal_map_parents(1),
    "goal_map_views3": goal_map_parents(3),
    "stg_masks": stg_masks,
    "stg_fields": stg_fields,
    "stg_scenes": stg_scenes,
    "roi": roi_inputs,
    "nms": nms_boxes(),
    "nms_one": nms_boxes((300,)),
    "paste": paste_inputs,
    "seg": seg_inputs,
}
