"""The tables behind tests/test_streams_gpu.py -- no GPU needed.

1. ``stream_cases.CONTRACT`` against include/peanut_hip.h: every prototype with a ``void* stream`` parameter has exactly one row, no
   row names a symbol that does not exist, every exemption carries a reason.  A stream-taking prototype added to the header without a
   row fails here.
2. Every "async" and "syncs" row is named, as a whole word, in tests/test_streams_gpu.py (the search of tests/test_options_cpu.py).
3. The input builders are deterministic, and the good and the stale input of every case differ."""
import ast
import os
import re

import torch

import stream_cases as sc
from test_abi import _declared_symbols

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _stream_prototypes():
    """Names of the prototypes of include/peanut_hip.h whose parameter list holds ``void* stream``."""
    with open(os.path.join(ROOT, "include", "peanut_hip.h"), encoding="utf-8") as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    out = []
    for m in re.finditer(r"\b(peanut_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", src, flags=re.S):
        if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2)):
            out.append(m.group(1))
    return out


def _word(symbol):
    return re.compile(r"(?<![A-Za-z0-9_])" + re.escape(symbol) + r"(?![A-Za-z0-9_])")


def test_every_stream_taking_prototype_has_exactly_one_contract_row():
    protos = _stream_prototypes()
    assert len(protos) == len(set(protos)) >= 34, protos
    assert set(protos) <= _declared_symbols()
    missing = sorted(set(protos) - set(sc.CONTRACT))
    assert not missing, f"prototypes that take a stream and have no CONTRACT row (class them from the header's words): {missing}"
    unknown = sorted(set(sc.CONTRACT) - set(protos))
    assert not unknown, f"CONTRACT rows that name no stream-taking prototype: {unknown}"
    # (a dict holds one row per key; the three source lists must not overlap either)
    assert len(sc._ASYNC) + len(sc._SYNCS) + len(sc._EXEMPT) == len(sc.CONTRACT)
    for symbol, (cls, reason) in sc.CONTRACT.items():
        assert cls in ("async", "syncs", "exempt"), symbol
        if cls == "exempt":
            assert isinstance(reason, str) and len(reason.split()) >= 3, f"{symbol}: an exemption needs a written reason"


def test_the_prototype_parser_sees_a_stream_parameter_and_nothing_else():
    protos = _stream_prototypes()
    assert "peanut_conv_forward" in protos and "peanut_stg_plan" in protos and "peanut_allgather_maps" in protos
    assert "peanut_conv_create" not in protos and "peanut_pred_probe_collect" not in protos and "peanut_stg_masks" not in protos


def test_the_header_states_the_class_of_every_synchronising_row():
    """The header's rule is "do not synchronise unless stated": every "syncs" row's own comment says so."""
    with open(os.path.join(ROOT, "include", "peanut_hip.h"), encoding="utf-8") as f:
        src = f.read()
    for symbol in sc._SYNCS:
        at = src.index(f" {symbol}(")
        comment = src[src.rindex("/*", 0, at):at]
        assert re.search(r"[Ss]ynchronises", comment), f"{symbol}: its comment does not say that it synchronises"
    for symbol in sc._ASYNC:
        at = src.index(f" {symbol}(")
        comment = src[src.rindex("/*", 0, at):at]
        assert not re.search(r"\bSynchronises\b|\bSynchronous\b", comment), f"{symbol}: classed async, but its comment says it synchronises"


def _code_only(source):
    """``source`` without comments and without docstrings (module, class, function): what is left names a symbol only where
    code uses the name."""
    tree = ast.parse(source)
    for node in ast.walk(tree):
        if isinstance(node, (ast.Module, ast.ClassDef, ast.FunctionDef, ast.AsyncFunctionDef)) and node.body and \
                isinstance(node.body[0], ast.Expr) and isinstance(getattr(node.body[0], "value", None), ast.Constant) and \
                isinstance(node.body[0].value.value, str):
            node.body[0] = ast.Pass()
    return ast.unparse(tree)


def test_the_code_only_view_drops_docstrings_and_comments():
    text = _code_only('"""peanut_a"""\nx = 1  # peanut_b\ndef f():\n    """peanut_c"""\n    return klass("peanut_d")\n')
    assert "peanut_d" in text and not any(s in text for s in ("peanut_a", "peanut_b", "peanut_c"))


def test_every_ordered_row_is_named_by_a_gpu_case():
    """The search runs over the CODE of tests/test_streams_gpu.py: its docstrings list every symbol and must not count."""
    with open(os.path.join(HERE, "test_streams_gpu.py"), encoding="utf-8") as f:
        text = _code_only(f.read())
    missing = [s for s, (cls, _) in sc.CONTRACT.items() if cls != "exempt" and not _word(s).search(text)]
    assert not missing, f"rows no case of tests/test_streams_gpu.py names: {missing}"
    assert _word("peanut_nms").search("lib.peanut_nms(x)") and not _word("peanut_nms").search("lib.peanut_nms_segments(x)")
    unused = [k for k in sc.INPUTS if not re.search(r'''["']''' + re.escape(k) + r'''["']''', text)]
    assert not unused, f"input builders no GPU case uses: {unused}"


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


def test_input_builders_are_deterministic_and_good_differs_from_stale():
    for name, build in sc.INPUTS.items():
        good, again, stale = build(0), build(0), build(1)
        assert _same(good, again), f"{name}: two builds of seed 0 differ"
        assert [(t.shape, t.dtype) for t in good] == [(t.shape, t.dtype) for t in stale], name
        assert not _same(good, stale), f"{name}: x_good equals x_stale"
        for t in good + stale:
            assert not t.dtype.is_floating_point or bool(torch.isfinite(t).all()), f"{name}: not valid data"


def test_conv_input_builders_are_deterministic_and_differ():
    """The conv cases build their inputs with ``stream_cases.randn`` over the shapes of ``conv_shapes`` (checked at batch 1: the
    batch only scales the first dimension)."""
    import test_streams_gpu as ts
    assert len(ts.CONV_CASES) >= 10
    for name, case in ts.CONV_CASES.items():
        c = case()
        shapes = ts.conv_shapes(c, 1)
        assert len(shapes) == 1 + bool(c["c2"]) + bool(c["residual"]) and c["B2"] > c["B"], name
        build = sc.randn(shapes)
        assert _same(build(0), build(0)) and not _same(build(0), build(1)), name
        assert [tuple(t.shape) for t in build(2)] == [tuple(s) for s in shapes], name


def test_the_backlog_is_bounded():
    assert 0 < sc.NOMINAL_MS <= sc.CAP_MS <= 200.0
