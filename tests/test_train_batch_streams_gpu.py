"""The stream contract of the training-batch calls (ABI 25).  Their streams travel in descriptors (``peanut_mapseq_train_t``,
``peanut_mapseq_bce_dense_t``), where the prototype check of tests/test_streams_cpu.py does not see them, so the rows the contract
table owes them are held here with the protocols of tests/stream_cases.py, as tests/test_mapio_streams_gpu.py does for ABI 21:
``peanut_mapseq_train_batch`` is "async" (ordered behind what is in flight on the caller's stream, returned while it is still
pending), ``peanut_mapseq_bce_dense`` "syncs" (it has read every input when it returns).  P1: late input, early overwrite; P2: back to
back, the second call of a larger shape."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_cases as sc              # noqa: E402
import train_batch_cases as tc         # noqa: E402

pytestmark = pytest.mark.gpu


def test_the_contract_table_cannot_see_the_two_calls():
    for symbol in ("peanut_mapseq_train_batch", "peanut_mapseq_bce_dense"):
        assert symbol not in sc.CONTRACT                       # (when it can, this file's rows move there)


def _seq(seed, shape=(3, 14, 47, 47)):
    return [torch.from_numpy(tc.make_sequence(shape[0], shape[1], shape[2:], seed)).cuda()]


def _params(n, pad, crop):
    from peanut_amd import mapio
    return mapio.TrainAugment(pad, crop, flip_prob=0.5, rotate_prob=0.5, seed=1).draw(n, crop)


def test_train_batch_is_ordered_on_the_callers_stream_and_does_not_wait():
    from peanut_amd import mapio

    def run(_, x, outs):
        S = x[0].shape[2]
        pad, crop = (S + 8, S + 4), (S - 3, S)
        return list(mapio.train_batch(x[0], [0, 2, 1, 0], _params(4, pad, crop), pad, crop, K=6))
    sc.p1("peanut_mapseq_train_batch", lambda: None, run, _seq(0), _seq(1), "async")
    sc.p2("peanut_mapseq_train_batch", lambda: None, run, [_seq(0), _seq(2, (3, 14, 96, 96)), _seq(3)])


def test_bce_dense_reads_its_inputs_behind_the_stream_and_before_it_returns():
    from peanut_amd import mapio

    def run(_, x, outs):
        return torch.from_numpy(mapio.bce_score_target(x[0], x[1]))

    def inputs(seed, S=47):
        g = torch.Generator().manual_seed(seed)
        gt = torch.from_numpy(tc.make_sequence(2, 6, (S, S), seed))
        return [(torch.randn((2, 6, S, S), generator=g) * 3).cuda(), gt.cuda()]
    sc.p1("peanut_mapseq_bce_dense", lambda: None, run, inputs(0), inputs(1), "syncs")
    sc.p2("peanut_mapseq_bce_dense", lambda: None, run, [inputs(0), inputs(2, 96), inputs(3)])
