"""The stream contract of ``peanut_pred_inference`` (ABI 24).  Its stream travels in the descriptor (``peanut_pred_infer_t``), where
the prototype check of tests/test_streams_cpu.py does not see it, so the row the contract table owes it is held here with the
protocols of tests/stream_cases.py: the call is "async" -- ordered behind what is in flight on the caller's stream (the gather, every
chunk's forward with its side-stream fork and the combine), returned while that is still pending; the window grid is host arithmetic
and nothing is read back.  P1: late input, early overwrite; P2: back to back on a fresh handle, the second call of a larger shape
(plans, workspace and both staging buffers are made and regrown under in-flight work)."""
import os
import re
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import infer_cases as ic               # noqa: E402
import stream_cases as sc              # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_header_states_the_class_of_the_call():
    with open(os.path.join(ROOT, "include", "peanut_hip.h"), encoding="utf-8") as f:
        src = f.read()
    assert "peanut_pred_inference" not in sc.CONTRACT          # (the table cannot see it; when it can, this file's row moves there)
    at = src.index("int peanut_pred_inference(")
    own = src[src.rindex("\n/* ", 0, at):at]
    assert re.search(r"No\s+synchronisation", own) and not re.search(r"\bSynchronises\b|\bSynchronous\b", own)
    assert "void* stream" not in src[at:src.index(";", at)]
    assert re.search(r"void\* stream;\s*\} peanut_pred_infer_t;", src)


def _make(max_batch=0):
    """A fresh model under case A's test_cfg with the pipeline's [none, horizontal] images."""
    def make():
        from peanut_amd.prediction import PEANUT_Prediction_Model
        from peanut_amd.weights import PredCfg, make_seeded_state_dict
        c = ic.CASES["A"]
        cfg = PredCfg(test_mode="slide", crop_size=c["crop"], stride=c["stride"], augs=((False, "horizontal"), (True, "horizontal")))
        m = PEANUT_Prediction_Model(SimpleNamespace(sem_gpu_id=0), state_dict=make_seeded_state_dict(PredCfg(), 0), cfg=cfg)
        m.max_batch = max_batch
        return m
    return make


def _run(m, x, outs):
    return m.model.inference(x[0], apply_sigmoid=True, max_batch=m.max_batch)


def _maps(seed, shape=None):
    if shape is None:
        return [ic.inputs("A", seed_offset=seed).cuda()]
    g = torch.Generator().manual_seed(31 * seed + 5)
    return [((torch.rand(shape, generator=g) > 0.7).float() * torch.rand(shape, generator=g)).cuda()]


def test_inference_is_ordered_on_the_callers_stream_and_does_not_wait():
    sc.p1("peanut_pred_inference", _make(), _run, _maps(0), _maps(1), "async")


def test_chunked_inference_is_ordered_on_the_callers_stream_and_does_not_wait():
    """max_batch = 4: fourteen forwards (the last of two maps, another plan) between the two glue launches."""
    sc.p1("peanut_pred_inference", _make(4), _run, _maps(0), _maps(1), "async")


def test_back_to_back_calls_on_a_fresh_handle():
    sc.p2("peanut_pred_inference", _make(), _run, [_maps(0), _maps(2, (2, 14, 72, 104)), _maps(3)])
