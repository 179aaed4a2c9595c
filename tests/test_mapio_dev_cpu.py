"""Map datasets on the device, without a GPU: the binding (ABI 21, the descriptors' layouts), the recorder's save-step
arithmetic, the dataset filter from sums, and the order in which ``evaluate`` lists files and samples."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from peanut_amd import _lib, mapio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_21_binds_the_three_entry_points_and_the_descriptors_match_the_header():
    assert _lib.ABI_VERSION >= 21
    lib = _lib.load()
    assert lib.peanut_abi_version() == _lib.ABI_VERSION
    for name in ("peanut_mapseq_encode", "peanut_mapseq_inputs", "peanut_mapseq_bce"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    # peanut_mapseq_t: a pointer, four int32 and the stream; peanut_mapseq_sample_t: three int32
    assert C.sizeof(_lib.MapSeqC) == 32 and C.sizeof(_lib.MapSeqSampleC) == 12
    assert [(n, getattr(_lib.MapSeqC, n).offset) for n, _ in _lib.MapSeqC._fields_] == \
        [("maps", 0), ("T", 8), ("C", 12), ("W", 16), ("H", 20), ("stream", 24)]
    # peanut_mapseq_encode_t: size, four int32, six pointers, the stream
    assert C.sizeof(_lib.MapSeqEncodeC) == 80
    assert [(n, getattr(_lib.MapSeqEncodeC, n).offset) for n, _ in _lib.MapSeqEncodeC._fields_] == \
        [("size", 0), ("E", 8), ("C", 12), ("W", 16), ("H", 20), ("src", 24), ("plane_stride", 32), ("row_stride", 40),
         ("col_stride", 48), ("dst", 56), ("sums", 64), ("stream", 72)]
    body = re.search(r"typedef struct \{([^}]*)\} peanut_mapseq_encode_t;", open(os.path.join(ROOT, "include", "peanut_hip.h")).read()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body)
    assert re.findall(r"(\w+)\s*[;,]", body) == [n for n, _ in _lib.MapSeqEncodeC._fields_]
    assert [(n, getattr(_lib.MapSeqSampleC, n).offset) for n, _ in _lib.MapSeqSampleC._fields_] == [("t_idx", 0), ("x1", 4), ("y1", 8)]
    src = open(os.path.join(ROOT, "include", "peanut_hip.h")).read()
    m = re.search(r"typedef struct \{\s*const uint8_t\* maps;\s*int32_t T, C, W, H;\s*void\* stream;\s*\} peanut_mapseq_t;", src)
    assert m, "peanut_mapseq_t changed: update _lib.MapSeqC"
    assert re.search(r"typedef struct \{\s*int32_t t_idx, x1, y1;\s*\} peanut_mapseq_sample_t;", src)
    assert int(re.search(r"#define PEANUT_MAPSEQ_MAX_BATCH (\d+)", src).group(1)) == _lib.MAPSEQ_MAX_BATCH == 16
    assert int(re.search(r"#define PEANUT_MAPSEQ_MAX_SAMPLES (\d+)", src).group(1)) == _lib.MAPSEQ_MAX_SAMPLES


def test_the_library_refuses_bad_arguments_before_it_touches_a_device():
    """Everything the three entry points refuse is refused on the host, from the arguments alone (no GPU here)."""
    lib = _lib.load()
    one = (C.c_void_p * 1)(4096)
    ll = lambda v: (C.c_longlong * 1)(v)
    size = C.sizeof(_lib.MapSeqEncodeC)
    enc = lambda E, Cn, cs=1, size=size: lib.peanut_mapseq_encode(C.byref(_lib.MapSeqEncodeC(
        size, E, Cn, 8, 8, one, ll(64), ll(8), ll(cs), one, 4096, None)))
    assert enc(0, 14) == -2 and enc(17, 14) == -2 and enc(1, 4) == -2 and enc(1, 14, cs=2) == -2 and enc(1, 14, size=size - 8) == -2
    seq = _lib.MapSeqC(4096, 3, 14, 47, 47, None)
    smp = lambda t, x, y: (_lib.MapSeqSampleC * 1)(_lib.MapSeqSampleC(t, x, y))
    inp = lambda t, x, y, S=16, B=1: lib.peanut_mapseq_inputs(C.byref(seq), smp(t, x, y), B, S, 4096)
    assert inp(0, 32, 0) == -2 and inp(0, 0, 32) == -2 and inp(0, -1, 0) == -2          # one cell over an edge
    assert inp(3, 0, 0) == -2 and inp(-1, 0, 0) == -2 and inp(0, 0, 0, S=48) == -2 and inp(0, 0, 0, B=65) == -2
    out = (C.c_double * 8)()
    bce = lambda K, x=0: lib.peanut_mapseq_bce(C.byref(seq), smp(0, x, 0), 1, 16, 4096, K, out)
    assert bce(11) == -2 and bce(0) == -2 and bce(6, x=32) == -2
    assert b"window" in lib.peanut_last_error()


class _State:
    """What the recorder reads of an Agent_State without a device: identity only (on_step is not reached on a non-save step)."""


def test_recorder_saves_after_the_act_when_i_plus_1_is_a_save_step():
    rec = mapio.MapSequenceRecorder([_State()])
    assert rec.save_steps == list(range(25, 525, 25))
    hits = [i for i in range(600) if rec.is_save_step(i)]
    assert hits == [s - 1 for s in mapio.SAVE_STEPS]                    # collect_maps.py:79-83: step_i += 1, then the test
    assert [rec._slot[i + 1] for i in hits] == list(range(20))          # seq_i
    rec = mapio.MapSequenceRecorder([_State()], save_steps=(2, 4, 5))
    assert [i for i in range(10) if rec.is_save_step(i)] == [1, 3, 4]
    rec.on_step(0, [rec.states[0]], [False])                            # not a save step: nothing is touched
    assert rec.launches == 0 and rec.sums(rec.states[0]) == (0, 0) and not rec.keep(rec.states[0])


def test_keep_from_sums_decides_as_keep_sequence():
    rng = np.random.RandomState(3)
    seen = set()
    for case in range(40):
        seq = np.zeros((4, 9, 12, 12), np.uint8)
        if case % 4:                                                    # explored mass on either side of the 4000 of :86
            n = rng.randint(1, 4 * 144)
            t, r, c = np.unravel_index(rng.choice(4 * 144, n, replace=False), (4, 12, 12))
            seq[t, 1, r, c] = rng.randint(1, 256, n)
        if case % 3:
            seq[rng.randint(4), 4 + rng.randint(5), rng.randint(12), rng.randint(12)] = rng.randint(1, 256)
        if case == 11:
            seq[:] = 0
            seq[0, 1, 0, :8] = seq[2, 1, 3, :8] = 250                           # exactly 4000: not kept (strictly greater)
            seq[1, 5, 0, 0] = 1
        sums = (int(np.sum(seq[:, 4:], dtype=np.uint64)), int(np.sum(seq[:, 1], dtype=np.uint64)))
        want = mapio.keep_sequence(seq)
        assert mapio.keep_from_sums(*sums) == want, (case, sums)
        seen.add(want)
        if case == 11:
            assert sums == (1, 4000) and not want
    assert seen == {True, False}


def test_evaluate_lists_files_by_name_and_ten_samples_per_file(tmp_path):
    (tmp_path / "val" / "b").mkdir(parents=True)
    for name in ("val/f00010.npz", "val/f00002.npz", "val/b/f00001.npz", "val/notes.txt"):
        (tmp_path / name).write_bytes(b"")
    root = str(tmp_path / "val")
    files = mapio.dataset_files(root)
    assert [os.path.relpath(f, root) for f in files] == ["b/f00001.npz", "f00002.npz", "f00010.npz"]
    assert mapio.dataset_files([files[2], files[0]]) == [files[0], files[2]]
    samples = mapio.dataset_samples(root)
    assert len(samples) == 30 and samples[:10] == [(files[0], t) for t in range(10)]      # train_prediction_model.py:155, 160
    assert samples == sorted(samples, key=lambda s: s[0])
    assert mapio.dataset_samples(files[1], (3, 1)) == [(files[1], 3), (files[1], 1)]
    with pytest.raises(ValueError):
        mapio.evaluate(type("M", (), {"device": "cpu"})(), [])         # no files: nothing to average
