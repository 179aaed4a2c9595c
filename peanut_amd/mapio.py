"""The reference's on-disk semantic-map sequence format: ``.npz`` with key
``maps`` = uint8 ``[T, 4+ncat, W, H]`` written by nav/collect_maps.py:67-68,80-87 (``full_map * 255``
truncated to uint8, 20 snapshots at steps 25, 50, ..., 500) and read back by
``LoadMapFromFile`` (prediction/train_prediction_model.py:63-68: ``maps[t_idx] / 255.``).  Lets real
PEANUT map datasets drive the benchmark / parity runs.

For HIP tensors the sequence lives on the device (csrc/mapio.hip, ABI 21): ``MapSequenceRecorder`` records the snapshots of
lock-step episodes as an ``on_step`` hook of ``replay.run_episode`` / ``run_episodes``, ``model_input_batch`` and ``bce_score``
make the model inputs and the reference's loss from an uploaded uint8 sequence, and ``evaluate`` scores a checkpoint on the
files of a dataset.  The host functions below are what they are held against.  ABI 25 adds the training side: ``MapStore`` keeps a
dataset on the device, ``TrainAugment`` draws the reference's augmentation parameters, ``train_batch`` / ``TrainBatcher`` build
augmented batches, input and target, in one launch."""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np
import torch

SAVE_STEPS = list(range(25, 525, 25))     # collect_maps.py:52


def encode_map(full_map) -> np.ndarray:
    """``(full_map.cpu().numpy() * 255).astype(np.uint8)`` (collect_maps.py:80-81; truncation).  HIP tensors take this host route
    too: the device route (``encode_maps_device(...)`` and a uint8 read-back, the same bits) took 0.54 [0.42, 0.62] ms against
    5.99 [5.29, 28.40] ms on a 960 x 960 x 14 map, but the host route's own spread on a shared host is larger than that gain
    (profiles/mapio/snapshot.jsonl), so it has not earned the default.  Callers that keep the snapshot on the
    device use ``encode_maps_device`` / ``MapSequenceRecorder``."""
    if isinstance(full_map, torch.Tensor):
        full_map = full_map.detach().cpu().numpy()
    return (full_map * 255).astype(np.uint8)


def keep_sequence(full_map_seq: np.ndarray) -> bool:
    """Dataset filter of collect_maps.py:86: some semantics seen and > 4000 explored cells."""
    return bool(np.sum(full_map_seq[:, 4:]) > 0 and np.sum(full_map_seq[:, 1]) > 4000)


def save_map_sequence(path: str, maps: Sequence) -> None:
    """np.savez_compressed(path, maps=uint8[T,C,W,H]) (collect_maps.py:87)."""
    seq = np.stack([m if isinstance(m, np.ndarray) and m.dtype == np.uint8 else encode_map(m) for m in maps])
    np.savez_compressed(path, maps=seq)


def load_map_sequence(path: str) -> np.ndarray:
    """uint8 [T,C,W,H]; accepts the .npz (key 'maps') and bare .npy forms LoadMapFromFile accepts
    (train_prediction_model.py:63-65)."""
    maps = np.load(path)
    if path[-1] == "z":
        maps = maps["maps"]
    return np.asarray(maps)


def model_input(maps: np.ndarray, t_idx: int, device=None) -> torch.Tensor:
    """float32 [1,C,W,H] in [0,1] (= ``maps[t_idx].astype(np.float32) / 255.``, :66-68) ready for
    ``PEANUT_Prediction_Model.get_prediction_batch``."""
    x = torch.from_numpy(maps[t_idx].astype(np.float32) / np.float32(255.0))[None]
    return x.to(device) if device is not None else x


def target_from_sequence(maps: np.ndarray, t_idx: int, goal_channels: Sequence[int] = range(4, 10)) -> np.ndarray:
    """Training target of the reference (train_prediction_model.py:85-89): last snapshot's goal
    channels masked to what is unexplored at ``t_idx``; uint8 [W,H,len(goal_channels)]."""
    img = maps[t_idx].transpose(1, 2, 0).astype(np.float32) / 255.
    mask = (img[:, :, 1] > 0)
    return (maps[-1, list(goal_channels)] * (1 - mask)).transpose(1, 2, 0)


# ---- the device side (csrc/mapio.hip) ----------------------------------------------------------------------------------------
def encode_maps_device(maps: Sequence[torch.Tensor], out: Optional[Sequence[torch.Tensor]] = None, sums: Optional[torch.Tensor] = None):
    """``peanut_mapseq_encode``: the snapshots of up to 16 episodes in one launch.  ``maps``: float32 [C,W,H] HIP tensors of one
    shape, read where they lie (views with a unit column stride are not copied); ``out``: contiguous uint8 [C,W,H] tensors
    (made when absent); ``sums``: int64 [E,2] on the device (made when absent), written whole: the sums of the bytes of channels
    ``4:`` and of channel 1 (the two terms of collect_maps.py:86).  Enqueued on the current stream; returns ``(out, sums)``."""
    from . import _lib
    maps = list(maps)
    E = len(maps)
    if not 1 <= E <= _lib.MAPSEQ_MAX_BATCH:
        raise ValueError(f"1..{_lib.MAPSEQ_MAX_BATCH} maps per launch, got {E}")
    for m in maps:
        if not (isinstance(m, torch.Tensor) and m.is_cuda and m.dtype == torch.float32 and m.dim() == 3):
            raise ValueError("every map must be a float32 [C,W,H] tensor on the HIP device")
    shape, dev = tuple(maps[0].shape), maps[0].device
    if any(tuple(m.shape) != shape or m.device != dev for m in maps):
        raise ValueError("the maps of one launch must have one shape and one device")
    maps = [m if m.stride(2) == 1 or m.shape[2] == 1 else m.contiguous() for m in maps]
    Cn, W, H = shape
    if out is None:
        out = [torch.empty(shape, dtype=torch.uint8, device=dev) for _ in maps]
    out = list(out)
    if len(out) != E or any(not isinstance(o, torch.Tensor) or o.dtype != torch.uint8 or tuple(o.shape) != shape or not o.is_contiguous() or o.device != dev for o in out):
        raise ValueError("out must be one contiguous uint8 [C,W,H] tensor per map")
    if len({o.data_ptr() for o in out}) != E:
        raise ValueError("two maps of one launch share one out tensor")
    if sums is None:
        sums = torch.empty((E, 2), dtype=torch.int64, device=dev)
    if sums.dtype != torch.int64 or tuple(sums.shape) != (E, 2) or not sums.is_contiguous() or sums.device != dev:
        raise ValueError("sums must be a contiguous int64 [E,2] tensor on the maps' device")
    lib = _lib.load()
    src = (C.c_void_p * E)(*[m.data_ptr() for m in maps])
    dst = (C.c_void_p * E)(*[o.data_ptr() for o in out])
    ps = (C.c_longlong * E)(*[m.stride(0) for m in maps])
    rs = (C.c_longlong * E)(*[m.stride(1) for m in maps])
    cs = (C.c_longlong * E)(*[1 if m.shape[2] == 1 else m.stride(2) for m in maps])
    d = _lib.MapSeqEncodeC(C.sizeof(_lib.MapSeqEncodeC), E, Cn, W, H, src, ps, rs, cs, dst, sums.data_ptr(), _lib.current_stream_ptr(dev))
    with torch.cuda.device(dev):
        rc = lib.peanut_mapseq_encode(C.byref(d))
    _lib.check(rc, "peanut_mapseq_encode")
    return out, sums


def keep_from_sums(sum_semantic: int, sum_explored: int) -> bool:
    """collect_maps.py:86 from the two sums of a whole sequence."""
    return bool(sum_semantic > 0 and sum_explored > 4000)


class MapSequenceRecorder:
    """What nav/collect_maps.py:67-87 does around the step loop, as the ``on_step`` hook of ``replay.run_episode`` /
    ``run_episodes``: ``rec = MapSequenceRecorder(states); run_episodes(states, ..., on_step=rec.on_step)``, then per state
    ``rec.save(state, path)``.

    After the step with index ``i``, when ``i + 1`` is a save step (:79-83 count after the act), ``state.full_map`` of every
    active episode is encoded as it is -- a local map not yet written back is not in the snapshot, as in the reference -- in one
    launch, into the episode's own zero-initialised uint8 [T,C,W,H] device buffer (an episode that ends early keeps zeros, as
    ``np.zeros`` does, :67).  The sums of the filter (:86) come out of the same pass, stay on the device until somebody asks and
    are accumulated as Python ints; ``keep`` decides from them, ``save`` copies an accepted sequence down once."""

    def __init__(self, states, save_steps: Sequence[int] = SAVE_STEPS):
        self.states = list(states)
        self.save_steps = [int(s) for s in save_steps]
        self._slot = {s: t for t, s in reversed(list(enumerate(self.save_steps)))}      # the first index of a repeated step
        self._index = {id(s): e for e, s in enumerate(self.states)}
        self._buf: List[Optional[torch.Tensor]] = [None] * len(self.states)
        self._sums = [[0, 0] for _ in self.states]
        self._pending: list = []
        self.launches = 0

    def reset(self) -> None:
        """Forget every recorded snapshot (before the states run their next episodes)."""
        for b in self._buf:
            if b is not None:
                b.zero_()
        self._sums = [[0, 0] for _ in self.states]
        self._pending = []

    def is_save_step(self, i: int) -> bool:
        return (i + 1) in self._slot

    def on_step(self, i, active_states, predicted=None) -> None:
        if not self.is_save_step(i):
            return
        t = self._slot[i + 1]
        act = list(active_states) if isinstance(active_states, (list, tuple)) else [active_states]
        from . import _lib
        for lo in range(0, len(act), _lib.MAPSEQ_MAX_BATCH):
            part = act[lo:lo + _lib.MAPSEQ_MAX_BATCH]
            idx = [self._index[id(s)] for s in part]
            srcs = [s.full_map for s in part]
            for e, m in zip(idx, srcs):
                if self._buf[e] is None:
                    self._buf[e] = torch.zeros((len(self.save_steps),) + tuple(m.shape), dtype=torch.uint8, device=m.device)
            _, sums = encode_maps_device(srcs, out=[self._buf[e][t] for e in idx])
            self._pending.append((idx, sums))
            self.launches += 1

    def _drain(self) -> None:
        for idx, sums in self._pending:
            for e, (a, b) in zip(idx, sums.cpu().tolist()):
                self._sums[e][0] += int(a)
                self._sums[e][1] += int(b)
        self._pending = []

    def sums(self, state):
        """(sum of the bytes of channels 4:, sum of the bytes of channel 1) over the recorded sequence, as Python ints."""
        self._drain()
        return tuple(self._sums[self._index[id(state)]])

    def keep(self, state) -> bool:
        """collect_maps.py:86, from the sums: the sequence is not touched."""
        return keep_from_sums(*self.sums(state))

    def sequence_device(self, state) -> Optional[torch.Tensor]:
        """The uint8 [T,C,W,H] device buffer of ``state`` (None before its first snapshot)."""
        return self._buf[self._index[id(state)]]

    def sequence(self, state) -> np.ndarray:
        """The recorded sequence on the host, uint8 [T,C,W,H] (one copy)."""
        buf = self.sequence_device(state)
        if buf is None:
            st = state.full_map
            return np.zeros((len(self.save_steps),) + tuple(st.shape), np.uint8)
        return buf.cpu().numpy()

    def save(self, state, path: str, force: bool = False) -> bool:
        """``if keep: np.savez_compressed(path, maps=full_map_seq)`` (:86-87).  A rejected sequence is neither copied nor
        written (``force`` writes it all the same); returns whether the file was written."""
        if not (force or self.keep(state)):
            return False
        np.savez_compressed(path, maps=self.sequence(state))
        return True


def to_device(maps: np.ndarray, device="cuda:0") -> torch.Tensor:
    """Upload a uint8 [T,C,W,H] sequence once, as it is stored."""
    maps = np.ascontiguousarray(maps)
    if maps.dtype != np.uint8 or maps.ndim != 4:
        raise ValueError(f"expected a uint8 [T,C,W,H] sequence, got {maps.dtype} {maps.shape}")
    return torch.from_numpy(maps).to(device)


def _samples(maps_dev: torch.Tensor, t_idx, window, origin):
    """The (t_idx, x1, y1) triples of a batch, checked on the host: ``t_idx`` an int or a sequence of them; ``window`` None = the
    whole (square) map; ``origin`` None = the centre crop of ``Agent_State._prediction_crop``, one ``(x1, y1)`` for all samples, or
    one pair per sample."""
    if not (isinstance(maps_dev, torch.Tensor) and maps_dev.is_cuda and maps_dev.dtype == torch.uint8 and maps_dev.dim() == 4
            and maps_dev.is_contiguous()):
        raise ValueError("maps_dev must be a contiguous uint8 [T,C,W,H] tensor on the HIP device (mapio.to_device)")
    T, Cn, W, H = maps_dev.shape
    ts = [int(t) for t in t_idx] if isinstance(t_idx, Iterable) else [int(t_idx)]
    if not ts:
        raise ValueError("no samples")
    if window is None:
        if W != H:
            raise ValueError(f"the map is {W} x {H}: give a window")
        window = W
    S = int(window)
    if origin is None:
        origin = (W // 2 - S // 2, H // 2 - S // 2)          # Agent_State._prediction_crop
    origin = np.asarray(origin, dtype=np.int64)
    if origin.ndim == 1:
        origin = np.broadcast_to(origin, (len(ts), 2))
    if origin.shape != (len(ts), 2):
        raise ValueError("origin must be (x1, y1) or one pair per sample")
    if S < 1:
        raise ValueError("the window must be positive")
    for b, (t, (x1, y1)) in enumerate(zip(ts, origin)):
        if not 0 <= t < T:
            raise ValueError(f"sample {b}: t_idx {t} outside [0, {T})")
        if x1 < 0 or y1 < 0 or x1 + S > W or y1 + S > H:
            raise ValueError(f"sample {b}: the {S} x {S} window at ({x1}, {y1}) leaves the {W} x {H} map")
    return ts, S, [(int(x), int(y)) for x, y in origin]


def _seq_desc(maps_dev):
    from . import _lib
    T, Cn, W, H = maps_dev.shape
    return _lib.MapSeqC(maps_dev.data_ptr(), T, Cn, W, H, _lib.current_stream_ptr(maps_dev.device))


def _sample_array(ts, origin, lo, hi):
    from . import _lib
    arr = (_lib.MapSeqSampleC * (hi - lo))()
    for k in range(lo, hi):
        arr[k - lo].t_idx, arr[k - lo].x1, arr[k - lo].y1 = ts[k], origin[k][0], origin[k][1]
    return arr


def model_input_batch(maps_dev: torch.Tensor, t_idx, window: Optional[int] = None, origin=None,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``model_input`` for a batch of samples of an uploaded sequence (``peanut_mapseq_inputs``): float32 [B,C,S,S] on the
    device, ``float(byte) / 255`` bit for bit, no host pass and no fp32 upload.  A window that leaves the map or a ``t_idx``
    outside the sequence raises ``ValueError`` before anything is enqueued."""
    from . import _lib
    ts, S, org = _samples(maps_dev, t_idx, window, origin)
    B, Cn, dev = len(ts), maps_dev.shape[1], maps_dev.device
    if out is None:
        out = torch.empty((B, Cn, S, S), dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B, Cn, S, S) or not out.is_contiguous() or out.device != dev:
        raise ValueError("out must be a contiguous float32 [B,C,S,S] tensor on the sequence's device")
    lib, seq = _lib.load(), _seq_desc(maps_dev)
    with torch.cuda.device(dev):
        for lo in range(0, B, _lib.MAPSEQ_MAX_SAMPLES):
            hi = min(B, lo + _lib.MAPSEQ_MAX_SAMPLES)
            rc = lib.peanut_mapseq_inputs(C.byref(seq), _sample_array(ts, org, lo, hi), hi - lo, S, out[lo:hi].data_ptr())
            _lib.check(rc, "peanut_mapseq_inputs")
    return out


def bce_score(logits: torch.Tensor, maps_dev: torch.Tensor, t_idx, window: Optional[int] = None, origin=None) -> np.ndarray:
    """The reference's loss (``my_loss``, train_prediction_model.py:173-184) of raw ``logits`` [B,K,S,S] against the target of
    :85-89 -- the last snapshot's channels ``4:4+K`` where channel 1 of snapshot ``t_idx`` is unexplored, ``/ 255.`` in fp32 --
    summed per sample and channel in float64 on the device (``peanut_mapseq_bce``); the target is never materialised.  Returns
    float64 [B,K] on the host (synchronises).  Divide by ``S * S`` for the mean."""
    from . import _lib
    ts, S, org = _samples(maps_dev, t_idx, window, origin)
    B = len(ts)
    if not (isinstance(logits, torch.Tensor) and logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 4):
        raise ValueError("logits must be a float32 [B,K,S,S] tensor on the HIP device")
    if logits.shape[0] != B or tuple(logits.shape[2:]) != (S, S) or logits.device != maps_dev.device:
        raise ValueError(f"logits {tuple(logits.shape)} do not match {B} samples of a {S} x {S} window")
    K = logits.shape[1]
    if not 1 <= K <= maps_dev.shape[1] - 4:
        raise ValueError(f"{K} logit channels, the sequence has {maps_dev.shape[1] - 4} semantic ones")
    logits = logits.contiguous()
    out = np.empty((B, K), np.float64)
    lib, seq, dev = _lib.load(), _seq_desc(maps_dev), maps_dev.device
    with torch.cuda.device(dev):
        for lo in range(0, B, _lib.MAPSEQ_MAX_SAMPLES):
            hi = min(B, lo + _lib.MAPSEQ_MAX_SAMPLES)
            part = np.empty((hi - lo, K), np.float64)
            rc = lib.peanut_mapseq_bce(C.byref(seq), _sample_array(ts, org, lo, hi), hi - lo, S, logits[lo:hi].data_ptr(), K,
                                       part.ctypes.data_as(C.POINTER(C.c_double)))
            _lib.check(rc, "peanut_mapseq_bce")
            out[lo:hi] = part
    return out


def dataset_files(paths) -> List[str]:
    """The files of a dataset in ``SemMapDataset.load_annotations``' order (train_prediction_model.py:150-160: every ``.npz`` under
    the directory, recursively, sorted by name).  ``paths``: a directory, a file, or a list of either."""
    if isinstance(paths, (str, os.PathLike)):
        paths = [paths]
    files = []
    for p in paths:
        p = os.fspath(p)
        if os.path.isdir(p):
            for root, _, names in os.walk(p):
                files += [os.path.join(root, n) for n in names if n.endswith(".npz")]
        else:
            files.append(p)
    return sorted(files)


def dataset_samples(paths, t_indices: Iterable[int] = range(10)) -> List[tuple]:
    """``[(file, t_idx)]`` as ``load_annotations`` lists them: per file ``t_idx`` in the given order (:155), files sorted by name
    (:160; Python's sort is stable, so the ``t_idx`` order within a file survives)."""
    ts = [int(t) for t in t_indices]
    return [(f, t) for f in dataset_files(paths) for t in ts]


# ---- augmented training batches (peanut_mapseq_train_batch, ABI 25) ----------------------------------------------------------
PARAMS_DTYPE = np.dtype([("off_r", np.int32), ("off_c", np.int32), ("flip", np.int32), ("rotate", np.int32), ("angle", np.float64)])
FLIP_CODES = {"horizontal": 1, "vertical": 2}     # horizontal = the last axis, vertical = the first map axis (mmcv.imflip on [W,H,C])


def _pair(v, what):
    v = (int(v), int(v)) if isinstance(v, (int, np.integer)) else tuple(int(x) for x in v)
    if len(v) != 2 or min(v) < 1:
        raise ValueError(f"{what} must be a positive size (rows, columns), got {v}")
    return v


class TrainAugment:
    """The random part of the reference's ``train_pipeline`` (nav/pred_model_cfg.py:47-56) -- ``Resize`` at ratio 1, ``Pad``,
    ``RandomCrop``, ``RandomFlip``, ``RandomRotate`` -- as parameter rows for ``train_batch``.  Owns a ``np.random.RandomState(seed)``
    and draws from it, per sample and in the reference's order (mmseg/datasets/pipelines/transforms.py:205, 603-604, 359, 706-707):
    ``random_sample()`` (Resize; consumed), ``randint(0, margin_r + 1)``, ``randint(0, margin_c + 1)``, ``rand()`` (flip),
    ``rand()`` and ``uniform(lo, hi)`` (rotation: both always drawn).  Under ``np.random.seed(seed)`` the reference's pipeline makes
    the same draws bit for bit."""

    def __init__(self, pad, crop, flip_prob=0.5, flip_direction="horizontal", rotate_prob=1.0, degree=180, seed=0):
        self.pad, self.crop = _pair(pad, "pad"), _pair(crop, "crop")
        if self.crop[0] > self.pad[0] or self.crop[1] > self.pad[1]:
            raise ValueError(f"the crop {self.crop} is larger than the pad {self.pad}")
        if flip_direction not in FLIP_CODES:
            raise ValueError(f"flip_direction must be 'horizontal' or 'vertical', got {flip_direction!r}")
        if not (0.0 <= float(flip_prob) <= 1.0 and 0.0 <= float(rotate_prob) <= 1.0):
            raise ValueError("probabilities must lie in [0, 1]")
        if isinstance(degree, (int, float)):
            if degree <= 0:
                raise ValueError(f"degree {degree} should be positive")
            degree = (-degree, degree)
        if len(degree) != 2:
            raise ValueError(f"degree {degree} should be a number or (min, max)")
        self.flip_prob, self.flip_code, self.flip_direction = float(flip_prob), FLIP_CODES[flip_direction], flip_direction
        self.rotate_prob, self.degree = float(rotate_prob), (min(*degree), max(*degree))
        self.seed = seed
        self.rng = np.random.RandomState(seed)

    @classmethod
    def identity(cls, map_shape, seed=0):
        """pad = crop = the map, no flip, no rotation: the batch is ``model_input_batch`` and the target of :85-89."""
        return cls(map_shape, map_shape, flip_prob=0.0, rotate_prob=0.0, seed=seed)

    @classmethod
    def from_pipeline(cls, cfg_list, seed=0):
        """From a ``train_pipeline`` list.  Exactly the reference's sequence is built: LoadMapFromFile, Resize, Pad, RandomCrop,
        RandomFlip, RandomRotate, then formatting (DefaultFormatBundle, Collect).  ``ValueError`` for what is not: a Resize
        ``ratio_range`` other than (1, 1) or an ``img_scale``, ``cat_max_ratio < 1``, ``size_divisor``, non-zero pad values, a
        RandomRotate ``center`` or ``auto_bound``, any other transform, another order."""
        want = ["Resize", "Pad", "RandomCrop", "RandomFlip", "RandomRotate"]
        got, kw = [], {}
        for cfg in cfg_list:
            cfg = dict(cfg)
            typ = cfg.pop("type", None)
            if typ in ("LoadMapFromFile", "DefaultFormatBundle", "Collect"):
                continue
            if typ not in want:
                raise ValueError(f"transform {typ!r} is not built")
            got.append(typ)
            if typ == "Resize":
                if cfg.get("img_scale") is not None:
                    raise ValueError("Resize with an img_scale is not built")
                rr = cfg.get("ratio_range")
                if rr is None or tuple(float(r) for r in rr) != (1.0, 1.0):
                    raise ValueError(f"Resize ratio_range {rr} is not built: only (1, 1)")
                if not cfg.get("keep_ratio", True) or cfg.get("min_size") is not None:
                    raise ValueError("Resize with keep_ratio=False or a min_size is not built")
            elif typ == "Pad":
                if cfg.get("size_divisor") is not None or cfg.get("size") is None:
                    raise ValueError("Pad needs a fixed size; size_divisor is not built")
                if cfg.get("pad_val", 0) != 0 or cfg.get("seg_pad_val", 255) != 0:
                    raise ValueError("Pad with non-zero pad values is not built (pad_val and seg_pad_val must be 0)")
                kw["pad"] = cfg["size"]
            elif typ == "RandomCrop":
                if cfg.get("cat_max_ratio", 1.0) < 1.0:
                    raise ValueError("RandomCrop with cat_max_ratio < 1 is not built")
                kw["crop"] = cfg["crop_size"]
            elif typ == "RandomFlip":
                prob = cfg.get("prob", cfg.get("flip_ratio"))       # (mmcv renames flip_ratio to prob)
                if prob is None:
                    raise ValueError("RandomFlip needs a prob")
                kw["flip_prob"], kw["flip_direction"] = prob, cfg.get("direction", "horizontal")
            else:
                if cfg.get("center") is not None or cfg.get("auto_bound", False):
                    raise ValueError("RandomRotate with a center or auto_bound is not built")
                if cfg.get("pad_val", 0) != 0 or cfg.get("seg_pad_val", 255) != 0:
                    raise ValueError("RandomRotate with non-zero pad values is not built (pad_val and seg_pad_val must be 0)")
                kw["rotate_prob"], kw["degree"] = cfg["prob"], cfg["degree"]
        if got != want:
            raise ValueError(f"the pipeline's transforms are {got}; built is exactly {want}")
        return cls(seed=seed, **kw)

    def draw(self, n, map_shape):
        """The parameter rows of ``n`` samples of ``map_shape`` = (W, H) maps: a ``PARAMS_DTYPE`` array (off_r, off_c, flip code,
        rotate 0 / 1, angle in degrees).  The angle is drawn, and kept, also where ``rotate`` is 0."""
        W, H = (int(v) for v in map_shape)
        if self.pad[0] < W or self.pad[1] < H:
            raise ValueError(f"the pad {self.pad} is smaller than the {W} x {H} map")         # (mmcv.impad asserts)
        rows = np.zeros(int(n), PARAMS_DTYPE)
        rng = self.rng
        for row in rows:
            rng.random_sample()                                                         # Resize: ratio_range (1, 1)
            row["off_r"] = rng.randint(0, self.pad[0] - self.crop[0] + 1)
            row["off_c"] = rng.randint(0, self.pad[1] - self.crop[1] + 1)
            row["flip"] = self.flip_code if rng.rand() < self.flip_prob else 0
            row["rotate"] = 1 if rng.rand() < self.rotate_prob else 0
            row["angle"] = rng.uniform(self.degree[0], self.degree[1])
        return rows


def rotation_terms(angle_deg):
    """(cos, sin) of an angle in degrees as ``train_batch`` hands them to the kernel (and tests/train_batch_cases.py restates)."""
    import math
    a = math.radians(float(angle_deg))
    return math.cos(a), math.sin(a)


def train_batch(seqs, t_idx, params, pad, crop, K=6, img=None, gt=None):
    """A training batch, input and target, by the reference's pipeline in one launch per 64 samples (``peanut_mapseq_train_batch``).
    ``seqs``: one uint8 [T,C,W,H] device tensor for all samples, or one per sample (of one C, W, H; T may differ); ``t_idx``: the
    snapshot per sample; ``params``: ``PARAMS_DTYPE`` rows (``TrainAugment.draw``); ``pad`` / ``crop``: (rows, columns).  Returns
    ``(img, gt)``: float32 [B,C,S_r,S_c] and uint8 [B,K,S_r,S_c] on the device, every element written; the target is the last
    snapshot's channels ``4:4+K`` where channel 1 of snapshot ``t_idx`` is unexplored.  Enqueued on the current stream."""
    from . import _lib
    ts = [int(t) for t in t_idx] if isinstance(t_idx, Iterable) else [int(t_idx)]
    B = len(ts)
    seqs = [seqs] * B if isinstance(seqs, torch.Tensor) else list(seqs)
    params = np.asarray(params)
    if B < 1 or len(seqs) != B or params.dtype != PARAMS_DTYPE or params.shape != (B,):
        raise ValueError("seqs, t_idx and params must name the same, positive number of samples (params: PARAMS_DTYPE rows)")
    for m in seqs:
        if not (isinstance(m, torch.Tensor) and m.is_cuda and m.dtype == torch.uint8 and m.dim() == 4 and m.is_contiguous()):
            raise ValueError("every sequence must be a contiguous uint8 [T,C,W,H] tensor on the HIP device (mapio.to_device)")
    dev, (Cn, W, H) = seqs[0].device, tuple(seqs[0].shape[1:])
    if any(m.device != dev or tuple(m.shape[1:]) != (Cn, W, H) for m in seqs):
        raise ValueError("the sequences of one batch must share C, W, H and the device")
    pad, crop = _pair(pad, "pad"), _pair(crop, "crop")
    K = int(K)
    if img is None:
        img = torch.empty((B, Cn) + crop, dtype=torch.float32, device=dev)
    elif img.dtype != torch.float32 or tuple(img.shape) != (B, Cn) + crop or not img.is_contiguous() or img.device != dev:
        raise ValueError("img must be a contiguous float32 [B,C,S_r,S_c] tensor on the sequences' device")
    if gt is None:
        gt = torch.empty((B, max(K, 0)) + crop, dtype=torch.uint8, device=dev)
    elif gt.dtype != torch.uint8 or tuple(gt.shape) != (B, K) + crop or not gt.is_contiguous() or gt.device != dev:
        raise ValueError("gt must be a contiguous uint8 [B,K,S_r,S_c] tensor on the sequences' device")
    lib = _lib.load()
    with torch.cuda.device(dev):
        for lo in range(0, B, _lib.MAPSEQ_MAX_SAMPLES):
            hi = min(B, lo + _lib.MAPSEQ_MAX_SAMPLES)
            arr = (_lib.MapSeqAugC * (hi - lo))()
            for k in range(lo, hi):
                a, p = arr[k - lo], params[k]
                a.maps, a.T, a.t_idx = seqs[k].data_ptr(), seqs[k].shape[0], ts[k]
                a.off_r, a.off_c, a.flip, a.rotate = int(p["off_r"]), int(p["off_c"]), int(p["flip"]), int(p["rotate"])
                a.cos_t, a.sin_t = rotation_terms(p["angle"])
            d = _lib.MapSeqTrainC(C.sizeof(_lib.MapSeqTrainC), hi - lo, Cn, W, H, pad[0], pad[1], crop[0], crop[1], K, 0, arr,
                                  img[lo:hi].data_ptr(), gt[lo:hi].data_ptr(), _lib.current_stream_ptr(dev))
            _lib.check(lib.peanut_mapseq_train_batch(C.byref(d)), "peanut_mapseq_train_batch")
    return img, gt


def bce_score_target(logits: torch.Tensor, gt: torch.Tensor) -> np.ndarray:
    """``bce_score`` against a given uint8 target [B,K,S_r,S_c] (the ``gt`` of ``train_batch``): the same loss, partition and order
    (``peanut_mapseq_bce_dense``), so the identity augmentation gives ``bce_score``'s bits.  Returns float64 [B,K] on the host
    (synchronises)."""
    from . import _lib
    if not (isinstance(logits, torch.Tensor) and logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 4):
        raise ValueError("logits must be a float32 [B,K,S_r,S_c] tensor on the HIP device")
    if not (isinstance(gt, torch.Tensor) and gt.dtype == torch.uint8 and gt.device == logits.device and tuple(gt.shape) == tuple(logits.shape)):
        raise ValueError(f"gt must be a uint8 tensor of the logits' shape {tuple(logits.shape)} and device")
    logits, gt = logits.contiguous(), gt.contiguous()
    B, K, Sr, Sc = logits.shape
    out = np.empty((B, K), np.float64)
    lib, dev = _lib.load(), logits.device
    with torch.cuda.device(dev):
        for lo in range(0, B, _lib.MAPSEQ_MAX_SAMPLES):
            hi = min(B, lo + _lib.MAPSEQ_MAX_SAMPLES)
            part = np.empty((hi - lo, K), np.float64)
            d = _lib.MapSeqBceDenseC(C.sizeof(_lib.MapSeqBceDenseC), hi - lo, K, Sr, Sc, logits[lo:hi].data_ptr(), gt[lo:hi].data_ptr(),
                                     part.ctypes.data_as(C.POINTER(C.c_double)), _lib.current_stream_ptr(dev))
            _lib.check(lib.peanut_mapseq_bce_dense(C.byref(d)), "peanut_mapseq_bce_dense")
            out[lo:hi] = part
    return out


def compact_sequence(maps: np.ndarray, t_indices: Iterable[int] = range(10)) -> np.ndarray:
    """What training reads of a stored sequence: the snapshots ``t_indices`` (in that order) followed by the last one, so that
    ``maps[-1]`` stays the target's source and sample ``t_indices[i]`` is snapshot ``i``.  A 20-snapshot file shrinks to 11."""
    ts = [int(t) for t in t_indices]
    if maps.ndim != 4 or any(not 0 <= t < maps.shape[0] for t in ts):
        raise ValueError(f"t_indices {ts} outside the sequence {maps.shape}")
    return np.ascontiguousarray(maps[ts + [maps.shape[0] - 1]])


class MapStore:
    """A dataset in device memory as the bytes it is stored in: every file of ``dataset_files(paths)`` is loaded once, compacted
    (``compact_sequence``) and uploaded.  ``samples``: ``[(file, t_idx)]`` in ``dataset_samples`` order; ``sample(i)`` gives the
    device sequence and the snapshot index within it.  Raises ``ValueError`` when the dataset exceeds ``max_bytes``."""

    def __init__(self, paths, device="cuda:0", t_indices: Iterable[int] = range(10), max_bytes: Optional[int] = None):
        self.t_indices = [int(t) for t in t_indices]
        self.files = dataset_files(paths)
        if not self.files:
            raise ValueError("no map files")
        self.device = torch.device(device)
        self.seqs: List[torch.Tensor] = []
        self.nbytes = 0
        for f in self.files:
            seq = compact_sequence(load_map_sequence(f), self.t_indices)
            if self.seqs and tuple(seq.shape[1:]) != tuple(self.seqs[0].shape[1:]):
                raise ValueError(f"{f}: maps of {seq.shape[1:]}, the dataset's are {tuple(self.seqs[0].shape[1:])}")
            self.nbytes += seq.nbytes
            if max_bytes is not None and self.nbytes > max_bytes:
                raise ValueError(f"the dataset exceeds max_bytes = {max_bytes} at {f} ({self.nbytes} bytes so far)")
            self.seqs.append(to_device(seq, self.device))
        self.samples = [(f, t) for f in self.files for t in self.t_indices]
        self.map_shape = tuple(self.seqs[0].shape[2:])
        self.channels = int(self.seqs[0].shape[1])

    def __len__(self):
        return len(self.samples)

    def sample(self, i):
        n = len(self.t_indices)
        return self.seqs[i // n], i % n


class TrainBatcher:
    """Batches of a ``MapStore`` under a ``TrainAugment``: iterating it walks ONE epoch of a seeded permutation of the samples
    (``np.random.RandomState(seed)``, a new permutation per epoch; the last batch of an epoch may be short), and every batch is
    ``{'img': float32 [B,C,S_r,S_c], 'gt_semantic_seg': uint8 [B,K,S_r,S_c], 'params': rows}`` on the device, one launch.
    ``batch_of(indices)`` builds the batch of the given samples (it draws their parameters)."""

    def __init__(self, store: MapStore, augment: TrainAugment, batch: int = 8, seed=0, K: int = 6):
        if batch < 1:
            raise ValueError("batch must be positive")
        self.store, self.augment, self.batch, self.K = store, augment, int(batch), int(K)
        self.rng = np.random.RandomState(seed)
        self.epoch = 0

    def __len__(self):
        return (len(self.store) + self.batch - 1) // self.batch

    def batch_of(self, indices) -> Dict:
        picks = [self.store.sample(int(i)) for i in indices]
        params = self.augment.draw(len(picks), self.store.map_shape)
        img, gt = train_batch([s for s, _ in picks], [t for _, t in picks], params, self.augment.pad, self.augment.crop, K=self.K)
        return {"img": img, "gt_semantic_seg": gt, "params": params}

    def __iter__(self):
        order = self.rng.permutation(len(self.store))
        self.epoch += 1
        for lo in range(0, len(order), self.batch):
            yield self.batch_of(order[lo:lo + self.batch])


def evaluate(model, paths, t_indices: Iterable[int] = range(10), window: Optional[int] = None, batch: Optional[int] = None,
             augment: Optional[TrainAugment] = None) -> Dict:
    """Score a prediction model on stored map sequences with the loss it was trained on.  Per file (``dataset_files``): upload the
    uint8 sequence once, build the inputs of its ``t_indices`` on the device, run ``model.get_prediction_batch(...,
    apply_sigmoid=False)`` in batches of ``batch`` (default: all samples of a file), score with ``bce_score``.  ``model``: a
    ``PEANUT_Prediction_Model``.  Returns ``loss`` (the mean over all cells: ``reduction='mean'``, weight 1.0),
    ``loss_per_channel`` [K] and ``n_maps``.

    ``augment``: a ``TrainAugment``: the loss under the training augmentation instead (how robust a checkpoint is to the shifts,
    flips and rotations it was trained with).  Files and batches are walked in the same order; per batch the route is
    ``TrainBatcher.batch_of`` -> forward -> ``bce_score_target``, the window is the augmentation's crop (``window`` must be None), and
    the identity augmentation returns what the plain call returns."""
    ts = [int(t) for t in t_indices]
    seg = getattr(model, "model", model)
    device = seg.device
    total, cells, n_maps = None, 0, 0
    if augment is not None and window is not None:
        raise ValueError("with an augmentation the window is its crop: give no window")
    for f in dataset_files(paths):
        step = len(ts) if not batch else int(batch)
        if augment is not None:
            batcher = TrainBatcher(MapStore([f], device, ts), augment, batch=step, K=seg.cfg.num_classes)
        else:
            maps_dev = to_device(load_map_sequence(f), device)
        for lo in range(0, len(ts), step):
            part = ts[lo:lo + step]
            if augment is not None:
                b = batcher.batch_of(range(lo, lo + len(part)))
                logits = seg.check_range(model.get_prediction_batch(b["img"], apply_sigmoid=False))
                sums = bce_score_target(logits, b["gt_semantic_seg"])
            else:
                x = model_input_batch(maps_dev, part, window)
                logits = seg.check_range(model.get_prediction_batch(x, apply_sigmoid=False))
                sums = bce_score(logits, maps_dev, part, window)
            total = sums.sum(axis=0) if total is None else total + sums.sum(axis=0)
            cells += len(part) * logits.shape[2] * logits.shape[3]
            n_maps += len(part)
    if total is None:
        raise ValueError("no map files")
    per_channel = total / cells
    return {"loss": float(per_channel.mean()), "loss_per_channel": [float(v) for v in per_channel], "n_maps": n_maps}
