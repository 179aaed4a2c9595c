"""Drop-in for ``nav/agent/mapping.py``: ``Semantic_Mapping(args)`` with the reference's call
signature and return tuple, executed by the HIP library (``peanut_map_*``); no CPU fallback."""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from . import _lib

_ARG_FIELDS = ("frame_height", "frame_width", "map_resolution", "map_size_cm", "global_downscaling",
               "vision_range", "hfov", "du_scale", "cat_pred_threshold", "exp_pred_threshold",
               "map_pred_threshold", "num_sem_categories", "camera_height")


class Semantic_Mapping(nn.Module):
    """``Semantic_Mapping`` (nav/agent/mapping.py:10-179).  ``args`` carries the fields the reference
    ctor reads (:15-37) plus ``device``.  ``forward`` keeps the reference's tensor contract:

        fp_map_pred [1,V,V], map_pred [C,M,M], pose_pred [3], current_pose [3]
            = sem_map_module(obs [1,C,h,w], pose_obs [3], maps_last [C,M,M], poses_last [3], agent_states)

    ``poses_last`` is updated IN PLACE and both returned poses alias it, exactly like the reference
    (its ``get_new_pose_batch`` mutates the view it is given, :143-160).  Everything stays on the
    device and is enqueued on the current stream; there is no host synchronisation."""

    def __init__(self, args):
        super().__init__()
        self.args = args
        self.device = getattr(args, "device", torch.device("cuda:0"))
        missing = [f for f in _ARG_FIELDS if not hasattr(args, f)]
        if missing:
            raise AttributeError(f"args is missing {missing}")
        if not torch.cuda.is_available():
            raise _lib.PeanutHipError("Semantic_Mapping needs a HIP device (no CPU fallback)")
        self._lib = _lib.load()
        c = _lib.MapCfgC()
        for f in _ARG_FIELDS:
            setattr(c, f, getattr(args, f))
        self.num_sem_categories = args.num_sem_categories
        self._h = C.c_void_p()
        with _lib.default_options(), torch.cuda.device(self.device):     # (the option lock: see _lib.default_options)
            _lib.check(self._lib.peanut_map_create(C.byref(self._h), C.byref(c)), "peanut_map_create")
        dims = (C.c_int * 4)()
        _lib.check(self._lib.peanut_map_dims(self._h, C.byref(dims)), "peanut_map_dims")
        self.channels, self.map_cells, self.vision_range, self.n_points = (int(d) for d in dims)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                self._lib.peanut_map_destroy(h)
                h.value = None       # (no attribute assignment: nn.Module.__setattr__ is gone at interpreter shutdown)
            except Exception:  # pragma: no cover
                pass

    @staticmethod
    def _chk(t, shape, name):
        if not (t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == tuple(shape)):
            raise ValueError(f"{name} must be a float32 HIP tensor of shape {tuple(shape)}, got "
                             f"{t.dtype} {tuple(t.shape)} on {t.device}")

    def use_graph(self, enable: bool = True):
        """Replay the ten launches of a step as one hipGraph per distinct set of buffers (captured on second use).
        Only effective when the caller passes persistent ``out=`` buffers (e.g. two map buffers used in turn)."""
        _lib.check(self._lib.peanut_map_use_graph(self._h, int(enable)), "peanut_map_use_graph")

    def forward(self, obs, pose_obs, maps_last, poses_last, agent_states=None, out=None):
        Cc, M, V = self.channels, self.map_cells, self.vision_range
        h, w = self.args.frame_height, self.args.frame_width
        self._chk(obs, (1, Cc, h, w), "obs")
        self._chk(pose_obs, (3,), "pose_obs")
        self._chk(maps_last, (Cc, M, M), "maps_last")
        self._chk(poses_last, (3,), "poses_last")
        if not poses_last.is_contiguous():
            raise ValueError("poses_last must be contiguous (it is updated in place)")
        obs, pose_obs, maps_last = obs.contiguous(), pose_obs.contiguous(), maps_last.contiguous()
        if out is None:
            fp_map_pred = torch.empty((1, V, V), dtype=torch.float32, device=obs.device)
            map_pred = torch.empty((Cc, M, M), dtype=torch.float32, device=obs.device)
        else:                                   # caller-owned (fp_map_pred, map_pred), must not alias maps_last
            fp_map_pred, map_pred = out
            self._chk(fp_map_pred, (1, V, V), "out[0]")
            self._chk(map_pred, (Cc, M, M), "out[1]")
            if not (fp_map_pred.is_contiguous() and map_pred.is_contiguous()):
                raise ValueError("out buffers must be contiguous")
        with torch.cuda.device(obs.device):
            rc = self._lib.peanut_map_forward(self._h, obs.data_ptr(), pose_obs.data_ptr(), maps_last.data_ptr(),
                                              poses_last.data_ptr(), fp_map_pred.data_ptr(), map_pred.data_ptr(),
                                              _lib.current_stream_ptr(obs.device))
        _lib.check(rc, "peanut_map_forward")
        return fp_map_pred, map_pred, poses_last, poses_last

    # ---- several episodes per step ----
    MAX_BATCH = 16      # PEANUT_MAP_MAX_BATCH

    def reserve(self, max_batch: int):
        """Allocate the scratch of ``forward_batch`` for up to ``max_batch`` episodes (``peanut_map_reserve``; synchronous, and
        the only allocation of the batched path).  A smaller or equal reserve is kept."""
        max_batch = int(max_batch)
        if not 1 <= max_batch <= self.MAX_BATCH:
            raise ValueError(f"max_batch must be 1..{self.MAX_BATCH}, got {max_batch}")
        with torch.cuda.device(self.device):
            _lib.check(self._lib.peanut_map_reserve(self._h, max_batch), "peanut_map_reserve")
        self.reserved = max(getattr(self, "reserved", 0), max_batch)

    def debug_launches(self) -> int:
        """Kernels enqueued by the last ``forward`` / ``forward_batch`` call of this module."""
        return int(self._lib.peanut_map_debug_launches(self._h))

    def forward_batch(self, obs, pose_obs, maps_last, poses_last, out=None):
        """``forward`` for E independent episodes in the launches of one single-episode step::

            fp_map_pred [E,V,V], [map_pred_e [C,M,M]], poses_last, poses_last
                = sem_map_module.forward_batch(obs [E,C,h,w], pose_obs [E,3], [maps_last_e [C,M,M]], poses_last [E,3])

        ``maps_last`` is a sequence of E tensors (every episode owns its map); ``poses_last`` is updated in place.  ``out`` =
        (fp_map_pred [E,V,V], [map_pred_e]) are caller-owned outputs, none of which may be one of ``maps_last``.  Per episode
        every output has the bits ``forward`` gives on the same inputs.  Needs ``reserve(E)`` (or more) first."""
        Cc, M, V = self.channels, self.map_cells, self.vision_range
        h, w = self.args.frame_height, self.args.frame_width
        if obs.dim() != 4:
            raise ValueError(f"obs must be [E,{Cc},{h},{w}], got {tuple(obs.shape)}")
        E = int(obs.shape[0])
        if not 1 <= E <= getattr(self, "reserved", 0):
            raise ValueError(f"forward_batch: E = {E} episodes, reserve() holds {getattr(self, 'reserved', 0)}")
        self._chk(obs, (E, Cc, h, w), "obs")
        self._chk(pose_obs, (E, 3), "pose_obs")
        self._chk(poses_last, (E, 3), "poses_last")
        if not poses_last.is_contiguous():
            raise ValueError("poses_last must be contiguous (it is updated in place)")
        maps_last = list(maps_last)
        if len(maps_last) != E:
            raise ValueError(f"maps_last holds {len(maps_last)} maps for {E} episodes")
        for e, m in enumerate(maps_last):
            self._chk(m, (Cc, M, M), f"maps_last[{e}]")
        obs, pose_obs = obs.contiguous(), pose_obs.contiguous()
        maps_last = [m.contiguous() for m in maps_last]
        if out is None:
            fp_map_pred = torch.empty((E, V, V), dtype=torch.float32, device=obs.device)
            map_pred = [torch.empty((Cc, M, M), dtype=torch.float32, device=obs.device) for _ in range(E)]
        else:
            fp_map_pred, map_pred = out
            map_pred = list(map_pred)
            self._chk(fp_map_pred, (E, V, V), "out[0]")
            if len(map_pred) != E:
                raise ValueError(f"out[1] holds {len(map_pred)} maps for {E} episodes")
            for e, m in enumerate(map_pred):
                self._chk(m, (Cc, M, M), f"out[1][{e}]")
            if not (fp_map_pred.is_contiguous() and all(m.is_contiguous() for m in map_pred)):
                raise ValueError("out buffers must be contiguous")
        last_p = (C.c_void_p * E)(*[m.data_ptr() for m in maps_last])
        pred_p = (C.c_void_p * E)(*[m.data_ptr() for m in map_pred])
        with torch.cuda.device(obs.device):
            rc = self._lib.peanut_map_forward_batch(self._h, E, obs.data_ptr(), pose_obs.data_ptr(), last_p, poses_last.data_ptr(),
                                                    fp_map_pred.data_ptr(), pred_p, _lib.current_stream_ptr(obs.device))
        _lib.check(rc, "peanut_map_forward_batch")
        return fp_map_pred, map_pred, poses_last, poses_last
