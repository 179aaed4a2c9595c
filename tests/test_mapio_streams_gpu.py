"""The stream contract of the map-dataset calls (ABI 21).  Their streams travel in descriptors (``peanut_mapseq_encode_t``,
``peanut_mapseq_t``), where the prototype check of tests/test_streams_cpu.py does not see them, so the rows the contract table owes
them are held here with the protocols of tests/stream_cases.py: ``peanut_mapseq_encode`` and ``peanut_mapseq_inputs`` are "async"
(ordered behind what is in flight on the caller's stream, returned while it is still pending), ``peanut_mapseq_bce`` "syncs" (it
has read every input when it returns).  P1: late input, early overwrite; P2: back to back, the second call of a larger shape."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_cases as sc              # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_header_states_the_class_of_the_three_calls():
    with open(os.path.join(ROOT, "include", "peanut_hip.h"), encoding="utf-8") as f:
        src = f.read()
    for symbol, pattern in (("peanut_mapseq_encode", r"No\s+synchronisation"), ("peanut_mapseq_inputs", r"No\s+synchronisation"),
                            ("peanut_mapseq_bce", r"Synchronises")):
        assert symbol not in sc.CONTRACT                       # (the table cannot see it; when it can, this file's rows move there)
        at = src.index(f"int {symbol}(")
        own = src[src.rindex("\n/* ", 0, at):at]                # the comment in front of the prototype (and of its descriptor)
        assert re.search(pattern, own), symbol
        assert "void* stream" not in src[at:src.index(";", at)]
    assert re.search(r"void\* stream;\s*\} peanut_mapseq_encode_t;", src) and re.search(r"void\* stream;\s*\} peanut_mapseq_t;", src)


def _maps(seed, shape=(14, 47, 47)):
    rng = np.random.RandomState(seed)
    return [torch.from_numpy(rng.uniform(0, 1, shape).astype(np.float32)).cuda() for _ in range(2)]


def _seq(seed, shape=(3, 14, 47, 47)):
    return [torch.from_numpy(np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8)).cuda()]


def test_encode_is_ordered_on_the_callers_stream_and_does_not_wait():
    from peanut_amd import mapio

    def run(_, x, outs):
        out, sums = mapio.encode_maps_device(x)
        return [out, sums]
    sc.p1("peanut_mapseq_encode", lambda: None, run, _maps(0), _maps(1), "async")
    sc.p2("peanut_mapseq_encode", lambda: None, run, [_maps(0), _maps(2, (14, 96, 96)), _maps(3)])


def test_inputs_are_ordered_on_the_callers_stream_and_do_not_wait():
    from peanut_amd import mapio

    def run(_, x, outs):
        return mapio.model_input_batch(x[0], [0, 2, 1], window=min(32, x[0].shape[2]))
    sc.p1("peanut_mapseq_inputs", lambda: None, run, _seq(0), _seq(1), "async")
    sc.p2("peanut_mapseq_inputs", lambda: None, run, [_seq(0), _seq(2, (3, 14, 96, 96)), _seq(3)])


def test_bce_reads_its_inputs_behind_the_stream_and_before_it_returns():
    from peanut_amd import mapio

    def run(_, x, outs):
        S = x[0].shape[2]
        return torch.from_numpy(mapio.bce_score(x[1][:, :, :S, :S].contiguous(), x[0], [0, 1], window=S))

    def inputs(seed, S=47):
        g = torch.Generator().manual_seed(seed)
        return _seq(seed, (3, 14, S, S)) + [(torch.randn((2, 6, 96, 96), generator=g) * 3).cuda()]
    sc.p1("peanut_mapseq_bce", lambda: None, run, inputs(0), inputs(1), "syncs")
    sc.p2("peanut_mapseq_bce", lambda: None, run, [inputs(0), inputs(2, 96), inputs(3)])
