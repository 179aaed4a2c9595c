"""The reference's on-disk semantic-map sequence format: ``.npz`` with key
``maps`` = uint8 ``[T, 4+ncat, W, H]`` written by nav/collect_maps.py:67-68,80-87 (``full_map * 255``
truncated to uint8, 20 snapshots at steps 25, 50, ..., 500) and read back by
``LoadMapFromFile`` (prediction/train_prediction_model.py:63-68: ``maps[t_idx] / 255.``).  Lets real
PEANUT map datasets drive the benchmark / parity runs.

For HIP tensors the sequence lives on the device (csrc/mapio.hip, ABI 21): ``MapSequenceRecorder`` records the snapshots of
lock-step episodes as an ``on_step`` hook of ``replay.run_episode`` / ``run_episodes``, ``model_input_batch`` and ``bce_score``
make the model inputs and the reference's loss from an uploaded uint8 sequence, and ``evaluate`` scores a checkpoint on the
files of a dataset.  The host functions below are what they are held against."""
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


def evaluate(model, paths, t_indices: Iterable[int] = range(10), window: Optional[int] = None, batch: Optional[int] = None) -> Dict:
    """Score a prediction model on stored map sequences with the loss it was trained on.  Per file (``dataset_files``): upload the
    uint8 sequence once, build the inputs of its ``t_indices`` on the device, run ``model.get_prediction_batch(...,
    apply_sigmoid=False)`` in batches of ``batch`` (default: all samples of a file), score with ``bce_score``.  ``model``: a
    ``PEANUT_Prediction_Model``.  Returns ``loss`` (the mean over all cells: ``reduction='mean'``, weight 1.0),
    ``loss_per_channel`` [K] and ``n_maps``."""
    ts = [int(t) for t in t_indices]
    seg = getattr(model, "model", model)
    device = seg.device
    total, cells, n_maps = None, 0, 0
    for f in dataset_files(paths):
        maps_dev = to_device(load_map_sequence(f), device)
        step = len(ts) if not batch else int(batch)
        for lo in range(0, len(ts), step):
            part = ts[lo:lo + step]
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
