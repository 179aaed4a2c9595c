"""The local planner's short-term goal on the HIP device: ctypes face of csrc/stg.hip.

``ShortTermGoal.get_stg`` is the reference's ``Agent_Helper._get_stg`` (nav/agent/agent_helper.py:374-493): planner traversible map,
dilated goal, geodesic field on the padded grid, the 11 x 11 window pick of ``FMMPlanner.get_short_term_goal``
(nav/agent/utils/fmm_planner.py:77-116), the eroded retry and the "make the goal larger" loop, all on the maps where they lie on
the device; the host reads back one 24-byte struct per solve.  The scalar state machine around it (``_plan`` :228-371: collision
bookkeeping, action choice, untrap) is ``peanut_amd.agent_helper.Agent_Helper``, which calls this class once per step and makes
``next_preset_goal()`` when ``last['retried']`` says it is due (:444-445); a caller that keeps its own planner does both itself.
There is no CPU fallback."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

MAX_RAD = 16      # PEANUT_STG_MAX_RAD
MAX_STEP = 5      # PEANUT_STG_MAX_STEP
MAX_BATCH = 16    # PEANUT_STG_MAX_BATCH


def stg_masks(sx: float, sy: float, step_size: int = 5):
    """``get_mask`` / ``get_dist`` (fmm_planner.py:8-36) for scale 1, as the library computes them on the host -> two float64
    [(2 step_size + 1)^2] arrays.  Needs no device."""
    size = 2 * int(step_size) + 1
    mask, dist = np.empty((size, size), np.float64), np.empty((size, size), np.float64)
    rc = _lib.load().peanut_stg_masks(float(sx), float(sy), int(step_size), mask.ctypes.data_as(C.POINTER(C.c_double)),
                                      dist.ctypes.data_as(C.POINTER(C.c_double)))
    _lib.check(rc, "peanut_stg_masks")
    return mask, dist


def _bounds(lmb):
    return (C.c_int * 4)(*[int(v) for v in lmb])


def stg_traversible(obstacle: torch.Tensor, full_wh, lmb, col_rad: int, collision, visited, start, erode: bool = False) -> torch.Tensor:
    """``peanut_stg_traversible``: the planner's traversible map, uint8 [(m + 2), (m + 2)].  ``obstacle`` is read where it lies
    (fp32, unit column stride; a view into a larger map is fine)."""
    if obstacle.dtype != torch.float32 or obstacle.dim() != 2 or obstacle.shape[0] != obstacle.shape[1] or obstacle.stride(1) != 1:
        raise ValueError(f"obstacle must be a square fp32 [m, m] tensor with unit column stride, got {tuple(obstacle.shape)} "
                         f"{obstacle.dtype} strides {tuple(obstacle.stride())}")
    dev, m = obstacle.device, int(obstacle.shape[0])
    out = torch.empty((m + 2, m + 2), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.load().peanut_stg_traversible(obstacle.data_ptr(), int(obstacle.stride(0)), m, int(full_wh[0]), int(full_wh[1]),
                                                C.byref(_bounds(lmb)), int(col_rad), int(bool(erode)),
                                                None if collision is None else collision.data_ptr(),
                                                None if visited is None else visited.data_ptr(), int(start[0]), int(start[1]),
                                                out.data_ptr(), _lib.current_stream_ptr(dev))
    _lib.check(rc, "peanut_stg_traversible")
    return out


def stg_goal(mask: torch.Tensor, radius: int, padded: bool = False) -> torch.Tensor:
    """``peanut_stg_goal``: the [m, m] goal map (or an already padded mask) dilated by disk(radius) inside the padded grid."""
    if mask.dtype != torch.uint8 or mask.dim() != 2 or mask.shape[0] != mask.shape[1] or not mask.is_contiguous():
        raise ValueError("the goal mask must be a contiguous square uint8 tensor")
    m = int(mask.shape[0]) - (2 if padded else 0)
    out = torch.empty((m + 2, m + 2), dtype=torch.uint8, device=mask.device)
    with torch.cuda.device(mask.device):
        rc = _lib.load().peanut_stg_goal(mask.data_ptr(), int(bool(padded)), m, int(radius), out.data_ptr(), _lib.current_stream_ptr(mask.device))
    _lib.check(rc, "peanut_stg_goal")
    return out


def stg_window(field: torch.Tensor, state, step_size: int = 5):
    """``peanut_stg_window``: ``get_short_term_goal(state)`` on a device field (float64 [n, n], contiguous) ->
    (stg_x, stg_y, distance, stop, replan) with the reference's types for scale 1.  One 24-byte read-back; synchronises."""
    if field.dtype != torch.float64 or field.dim() != 2 or field.shape[0] != field.shape[1] or not field.is_contiguous():
        raise ValueError("the field must be a contiguous square float64 tensor")
    dev = field.device
    res = torch.empty(C.sizeof(_lib.StgWindowC), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.load().peanut_stg_window(field.data_ptr(), int(field.shape[0]), float(state[0]), float(state[1]), int(step_size),
                                           res.data_ptr(), _lib.current_stream_ptr(dev))
    _lib.check(rc, "peanut_stg_window")
    w = _lib.StgWindowC.from_buffer_copy(res.cpu().numpy().tobytes())
    return float(w.stg_r), float(w.stg_c), np.float64(w.distance), bool(w.stop), bool(w.replan)


class ShortTermGoal:
    """peanut_stg_t: the padded masks, the field and the solver for one local-map size.  ``args`` supplies ``map_size_cm``,
    ``map_resolution``, ``global_downscaling``, ``col_rad`` and (optional, default 100) ``magnify_goal_when_hard``."""

    def __init__(self, args, device="cuda:0", step_size: int = 5):
        if not torch.cuda.is_available():
            raise _lib.PeanutHipError("the short-term goal needs a HIP device (no CPU fallback)")
        self._lib = _lib.load()
        self.args = args
        self.device = torch.device(device)
        self.full_w = self.full_h = int(args.map_size_cm // args.map_resolution)
        self.m = int(self.full_w / args.global_downscaling)
        self.col_rad = int(args.col_rad)
        self.step_size = int(step_size)
        self.last = None
        self._h = C.c_void_p()
        with _lib.default_options(), torch.cuda.device(self.device):      # (the option lock: _lib.default_options)
            _lib.check(self._lib.peanut_stg_create(C.byref(self._h), self.m, self.full_w, self.full_h, self.col_rad, self.step_size),
                       "peanut_stg_create")

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                self._lib.peanut_stg_destroy(h)
            except Exception:  # pragma: no cover
                pass
            self._h = C.c_void_p()

    @property
    def waves(self) -> int:
        """``peanut_stg_waves``: the synchronising waves of the last plan this handle took part in."""
        return int(self._lib.peanut_stg_waves(self._h))

    def _check(self, obstacle, goal_map, collision_map, visited_vis):
        for name, t, dt in (("obstacle", obstacle, torch.float32), ("goal_map", goal_map, torch.uint8),
                            ("collision_map", collision_map, torch.uint8), ("visited_vis", visited_vis, torch.uint8)):
            if not isinstance(t, torch.Tensor) or t.dtype != dt or t.device != self.device or t.dim() != 2 or t.stride(1) != 1:
                raise ValueError(f"{name} must be a 2-D {dt} tensor on {self.device} with unit column stride")
        m = self.m
        if tuple(obstacle.shape) != (m, m) or tuple(goal_map.shape) != (m, m) or not goal_map.is_contiguous():
            raise ValueError(f"obstacle and goal_map must be [{m}, {m}] (goal_map contiguous)")
        for name, t in (("collision_map", collision_map), ("visited_vis", visited_vis)):
            if tuple(t.shape) != (self.full_w, self.full_h) or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous [{self.full_w}, {self.full_h}] tensor")

    def _set_last(self, res, tap):
        self.last = dict(stg=(float(res.stg_x), float(res.stg_y)), distance=float(res.distance), stop=bool(res.stop), replan=bool(res.replan),
                         retried=int(res.retried), n_magnify=int(res.n_magnify), n_solves=int(res.n_solves))
        if tap[0] is not None:
            self.last.update(trav=tap[0], goal=tap[1], dist=tap[2])
        return self.last["stg"], self.last["stop"]

    def get_stg(self, obstacle, goal_map, collision_map, visited_vis, lmb, start_exact, found_goal, goal_name, taps: bool = False):
        """``_get_stg(grid, start, goal, planning_window)`` -> ((stg_x, stg_y), stop).  obstacle: fp32 [m, m] (``local_map[0]``, read
        in place); goal_map: uint8 [m, m]; collision_map / visited_vis: uint8 [full_w, full_h]; ``.last`` keeps the whole result
        (with ``taps``: also the last solve's ``trav``, ``goal`` and ``dist`` tensors)."""
        self._check(obstacle, goal_map, collision_map, visited_vis)
        m = self.m
        is_toilet = goal_name == 'toilet'                                  # smaller radius and fewer steps for a toilet (:427-430, :479)
        found = 1 if found_goal == 1 else 0
        start = (C.c_double * 2)(float(start_exact[0]), float(start_exact[1]))
        res = _lib.StgResultC()
        n = m + 2
        tap = [torch.empty((n, n), dtype=dt, device=self.device) for dt in (torch.uint8, torch.uint8, torch.float64)] if taps else [None] * 3
        with torch.cuda.device(self.device):
            rc = self._lib.peanut_stg_plan(self._h, obstacle.data_ptr(), int(obstacle.stride(0)), goal_map.data_ptr(), collision_map.data_ptr(),
                                           visited_vis.data_ptr(), C.byref(_bounds(lmb)), C.byref(start), found, 6 if is_toilet else 8,
                                           float(getattr(self.args, "magnify_goal_when_hard", 100)), 2 if is_toilet else 8, C.byref(res),
                                           *[None if t is None else t.data_ptr() for t in tap], _lib.current_stream_ptr(self.device))
        _lib.check(rc, "peanut_stg_plan")
        return self._set_last(res, tap)


def get_stg_batch(planners, inputs, taps: bool = False):
    """``ShortTermGoal.get_stg`` for E planners in one ``peanut_stg_plan_batch``: the launches and synchronisations of the longest
    chain among the episodes instead of those of all chains in a row.  ``inputs``: E tuples ``(obstacle, goal_map, collision_map,
    visited_vis, lmb, start_exact, found_goal, goal_name)`` -> E ``((stg_x, stg_y), stop)`` pairs, every one the bits of the single
    call; each planner's ``.last`` is set as the single call sets it.  ``ValueError``: an empty batch, more than ``MAX_BATCH``
    episodes, planners of different sizes, devices, collision radii or step sizes, a planner named twice, a bad tensor."""
    planners, inputs = list(planners), [tuple(i) for i in inputs]
    E = len(planners)
    if E < 1 or E > MAX_BATCH:
        raise ValueError(f"get_stg_batch takes 1..{MAX_BATCH} episodes, got {E}")
    if len(inputs) != E or any(len(i) != 8 for i in inputs):
        raise ValueError("get_stg_batch needs one tuple of the eight get_stg arguments per planner")
    p0 = planners[0]
    if len({id(p) for p in planners}) != E:
        raise ValueError("the same planner appears twice")
    for e, p in enumerate(planners):
        if (p.device, p.m, p.full_w, p.full_h, p.col_rad, p.step_size) != (p0.device, p0.m, p0.full_w, p0.full_h, p0.col_rad, p0.step_size):
            raise ValueError(f"planner {e} differs from planner 0 in device, map sizes, col_rad or step_size: a mixed batch")
        p._check(*inputs[e][:4])
        if len(inputs[e][4]) != 4 or len(inputs[e][5]) != 2:
            raise ValueError(f"episode {e}: lmb must hold four boundaries and start_exact two coordinates")
    n = p0.m + 2
    toilet = [i[7] == 'toilet' for i in inputs]
    tap = [[torch.empty((n, n), dtype=dt, device=p0.device) for dt in (torch.uint8, torch.uint8, torch.float64)] if taps else [None] * 3
           for _ in range(E)]
    ptrs = lambda vals: (C.c_void_p * E)(*vals)
    ints = lambda vals: (C.c_int * E)(*[int(v) for v in vals])
    res = (_lib.StgResultC * E)()
    keep = dict(
        h=ptrs([p._h.value for p in planners]), obstacle=ptrs([i[0].data_ptr() for i in inputs]),
        row_stride=(C.c_longlong * E)(*[int(i[0].stride(0)) for i in inputs]), goal_map=ptrs([i[1].data_ptr() for i in inputs]),
        collision=ptrs([i[2].data_ptr() for i in inputs]), visited=ptrs([i[3].data_ptr() for i in inputs]),
        lmb=(C.c_int * (4 * E))(*[int(v) for i in inputs for v in i[4]]),
        start_exact=(C.c_double * (2 * E))(*[float(v) for i in inputs for v in i[5]]),
        found_goal=ints([1 if i[6] == 1 else 0 for i in inputs]), radius_found=ints([6 if t else 8 for t in toilet]),
        magnify_when_hard=(C.c_double * E)(*[float(getattr(p.args, "magnify_goal_when_hard", 100)) for p in planners]),
        max_magnify=ints([2 if t else 8 for t in toilet]))
    desc = _lib.StgBatchC(size=C.sizeof(_lib.StgBatchC), E=E, reserved=0, result_out=res, **keep)
    if taps:
        tap_arrays = [ptrs([tap[e][k].data_ptr() for e in range(E)]) for k in range(3)]
        desc.trav_out, desc.goal_out, desc.dist_out = tap_arrays
    with torch.cuda.device(p0.device):
        desc.stream = _lib.current_stream_ptr(p0.device)
        rc = p0._lib.peanut_stg_plan_batch(C.byref(desc))
    _lib.check(rc, "peanut_stg_plan_batch")
    return [p._set_last(res[e], tap[e]) for e, p in enumerate(planners)]
