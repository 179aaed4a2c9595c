"""The option surface of the library (csrc/options.h) as a whole -- no GPU needed: the option table is host code.

1. The guard: every key ``peanut_option_list()`` names is set by at least one test.  An option is a second code path behind a
   documented PEANUT_<KEY> environment variable; a path no test has ever run may compute anything.  The check is textual -- the
   key as a whole word in some tests/*.py other than this file -- which is what a reviewer would grep for; the tests that set a
   key assert the path it selects (tests/test_option_paths_gpu.py, tests/test_option_policy_gpu.py, the goal solver's files).
2. The plumbing every one of those tests relies on: peanut_set_default_option / peanut_get_default_option round-trip every key in
   both spellings, and ``_lib.default_options`` puts every value back."""
import ctypes as C
import glob
import os
import re

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

# key -> why no test sets it.  Starts empty: an option added without a test fails the suite.  No kernel-selecting option belongs here.
EXEMPT = {}


def _keys():
    from peanut_amd import _lib
    text = _lib.load().peanut_option_list().decode()
    keys = [line.split("=", 1)[0] for line in text.splitlines() if line.strip()]
    assert keys and all(re.fullmatch(r"[a-z][a-z0-9_]*", k) for k in keys), keys
    assert len(set(keys)) == len(keys)
    return keys


def _defaults():
    from peanut_amd import _lib
    text = _lib.load().peanut_option_list().decode()
    out = {}
    for line in text.splitlines():
        if line.strip():
            k, rest = line.split("=", 1)
            out[k] = int(rest.split(" ", 1)[0])
    return out


def test_every_option_is_set_by_some_test():
    keys = _keys()
    assert len(keys) >= 59
    sources = {}
    for path in sorted(glob.glob(os.path.join(HERE, "*.py"))):
        if os.path.basename(path) == os.path.basename(__file__):
            continue
        with open(path, encoding="utf-8") as f:
            sources[os.path.basename(path)] = f.read()
    assert sources
    unknown = sorted(set(EXEMPT) - set(keys))
    assert not unknown, f"exempted keys that are no options: {unknown}"
    assert all(isinstance(r, str) and len(r.split()) >= 3 for r in EXEMPT.values()), "an exemption needs a written reason"
    missing = []
    for k in keys:
        if k in EXEMPT:
            continue
        word = re.compile(r"(?<![A-Za-z0-9_])" + re.escape(k) + r"(?![A-Za-z0-9_])")
        if not any(word.search(text) for text in sources.values()):
            missing.append(k)
    assert not missing, f"options no test sets (add a test that asserts the path they select, or a reasoned exemption): {missing}"


def test_the_guard_sees_a_key_only_as_a_whole_word():
    """`pw256_mink` must not count as a test of `pw256_min` (nor of `w256_mink`): the lookarounds of the guard's pattern."""
    word = re.compile(r"(?<![A-Za-z0-9_])" + re.escape("nchunk") + r"(?![A-Za-z0-9_])")
    assert word.search('options={"nchunk": 3}') and word.search("default_options(nchunk=0)")
    assert not word.search("nchunks = 4") and not word.search("p.nchunk_x") and not word.search("innchunk")


def test_default_option_round_trip_in_both_spellings():
    """set -> get returns the value under `key` and `PEANUT_KEY` alike (case-insensitive, options.h: option_index), touches no
    other key, and an unknown key is refused by both calls."""
    from peanut_amd import _lib
    lib = _lib.load()
    keys = _keys()

    def get(name):
        v = C.c_longlong(-12345)
        assert lib.peanut_get_default_option(name.encode(), C.byref(v)) == 0, name
        return v.value

    with _lib.default_options():                      # the option lock: no handle is created on another thread meanwhile
        before = {k: get(k) for k in keys}
        try:
            for n, k in enumerate(keys):
                env = "PEANUT_" + k.upper()
                assert get(env) == before[k]
                for name, val in ((k, 1000 + n), (env, -7 - n), (k.upper(), 3)):
                    assert lib.peanut_set_default_option(name.encode(), val) == 0, name
                    assert get(k) == val and get(env) == val, (name, val)
                others = {o: get(o) for o in keys if o != k}
                assert others == {o: before[o] for o in keys if o != k}, f"setting {k} changed another option"
                assert lib.peanut_set_default_option(k.encode(), before[k]) == 0
        finally:
            for k, v in before.items():
                lib.peanut_set_default_option(k.encode(), v)
        assert {k: get(k) for k in keys} == before
        for bad in ("no_such_option", "PEANUT_", "", "pw256_mink "):
            v = C.c_longlong(5)
            assert lib.peanut_set_default_option(bad.encode(), 1) != 0, bad
            assert lib.peanut_get_default_option(bad.encode(), C.byref(v)) != 0 and v.value == 5, bad
        assert {k: get(k) for k in keys} == before


def test_default_options_block_restores_every_value():
    """``with default_options(k=v)``: the value holds inside the block and the earlier one is back after it -- after a normal exit,
    after an exception, and when a later key of the same block is refused (the keys before it are put back).  Without a PEANUT_<KEY>
    variable in the environment the earlier value is the built-in default the option list prints."""
    from peanut_amd import _lib
    lib = _lib.load()
    keys = _keys()
    builtin = _defaults()

    def get(name):
        v = C.c_longlong()
        assert lib.peanut_get_default_option(name.encode(), C.byref(v)) == 0
        return v.value

    before = {k: get(k) for k in keys}
    for k in keys:
        if "PEANUT_" + k.upper() not in os.environ:
            assert before[k] == builtin[k], k
    with _lib.default_options(**{k: before[k] + 11 for k in keys}):
        assert {k: get(k) for k in keys} == {k: before[k] + 11 for k in keys}
        with _lib.default_options(**{keys[0]: 5}):    # re-entrant, innermost value wins
            assert get(keys[0]) == 5
        assert get(keys[0]) == before[keys[0]] + 11
    assert {k: get(k) for k in keys} == before
    with pytest.raises(ZeroDivisionError):
        with _lib.default_options(**{k: 2 for k in keys}):
            assert get(keys[-1]) == 2
            1 / 0
    assert {k: get(k) for k in keys} == before
    with pytest.raises(_lib.PeanutHipError):
        with _lib.default_options(**{keys[0]: 9, keys[1]: 9, "no_such_option": 1}):
            pass
    assert {k: get(k) for k in keys} == before
