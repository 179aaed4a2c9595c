"""The poison switch of the library's own allocations (csrc/options.h: debug_poison_alloc) and the helpers of
tests/test_workspace_gpu.py that need no GPU."""
import ctypes as C

import numpy as np
import torch

from peanut_amd import _lib
from workspace_cases import first_difference, same


def test_debug_poison_alloc_is_listed_defaults_to_off_and_round_trips():
    lib = _lib.load()
    lines = lib.peanut_option_list().decode().splitlines()
    mine = [ln for ln in lines if ln.startswith("debug_poison_alloc=")]
    assert len(mine) == 1 and mine[0].startswith("debug_poison_alloc=0") and "[create-time]" not in mine[0], mine
    v = C.c_longlong(-7)
    _lib.check(lib.peanut_get_default_option(b"debug_poison_alloc", C.byref(v)))
    assert v.value == 0
    try:
        _lib.check(lib.peanut_set_default_option(b"debug_poison_alloc", 1))
        _lib.check(lib.peanut_get_default_option(b"PEANUT_DEBUG_POISON_ALLOC", C.byref(v)))      # the env-style spelling, same option
        assert v.value == 1
    finally:
        _lib.check(lib.peanut_set_default_option(b"debug_poison_alloc", 0))
    with _lib.default_options(debug_poison_alloc=1):
        _lib.check(lib.peanut_get_default_option(b"debug_poison_alloc", C.byref(v)))
        assert v.value == 1
    _lib.check(lib.peanut_get_default_option(b"debug_poison_alloc", C.byref(v)))
    assert v.value == 0


def test_same_is_bit_equality_over_every_field():
    nan = float("nan")
    a = dict(goal=(3, 4), value_max=nan, kept=False, dist=torch.tensor([1.0, nan, float("inf")], dtype=torch.float64),
             inst=[dict(boxes=torch.zeros(2, 4), masks=None)], arr=np.array([0.5, nan], np.float32))
    b = dict(goal=(3, 4), value_max=nan, kept=False, dist=torch.tensor([1.0, nan, float("inf")], dtype=torch.float64),
             inst=[dict(boxes=torch.zeros(2, 4), masks=None)], arr=np.array([0.5, nan], np.float32))
    assert same(a, b)
    for key, other in [("goal", (3, 5)), ("value_max", 0.0), ("kept", True), ("dist", torch.tensor([1.0, 2.0, float("inf")], dtype=torch.float64)),
                       ("dist", torch.tensor([1.0, nan, float("inf")])), ("inst", [dict(boxes=torch.zeros(2, 4), masks=torch.zeros(0))]),
                       ("inst", []), ("arr", np.array([0.5, 0.0], np.float32))]:
        c = dict(b)
        c[key] = other
        assert not same(a, c), key
        assert key in first_difference(a, c)
    assert not same(torch.tensor([0.0]), torch.tensor([-0.0]))          # bits, not values
    assert not same((1, 2), [1, 2]) and not same(dict(a=1), dict(b=1)) and not same(1, 1.0)
