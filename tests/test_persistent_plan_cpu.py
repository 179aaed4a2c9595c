"""The tail plan of the persistent pointwise kernels (peanut_amd/csrc/persistent_plan.h) against the plans the two launchers
computed before they shared it.

tests/golden/persistent_plans.json holds (as the sweep's axes plus an index into the distinct plans) what the former
``launch_conv_pw256p`` / ``launch_conv_pw256wp`` blocks gave over a sweep of tile counts, grid sizes, k-tile counts, scratch sizes, stream-K on / off and (256 x 128) the two-level accumulation;
tests/c_abi/plan_host.cpp prints the same sweep from the shared function.  Every field must be equal, and every plan that
fits must keep the invariants the kernels rely on.  No GPU: the header is plain C++17.
"""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["kernel", "T", "G", "nkt", "ws_floats", "streamk", "flush", "n_full", "n_sp", "split_p", "sk_units", "sk_maxp", "sk_g",
          "sk_q", "status"]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail("no system C++ compiler (c++ / g++ / clang++) to build tests/c_abi/plan_host.cpp")
    exe = str(tmp_path_factory.mktemp("plan") / "plan_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "peanut_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c_abi", "plan_host.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()
    head = out[0].split()
    assert head[0] == "kMaxItems"
    rows = []
    for line in out[1:]:
        f = line.split()
        row = {"kernel": f[0], "status": f[14]}
        for name, v in zip(FIELDS[1:14], f[1:14]):
            row[name] = int(v)
        row["part_tiles"], row["tile_floats"], row["dump"] = int(f[15]), int(f[16]), int(f[17])
        rows.append(row)
    return int(head[1]), rows


@pytest.fixture(scope="module")
def golden():
    """The recorded rows, expanded from the file's compact form (the sweep's axes + an index into the distinct plans)."""
    with open(os.path.join(ROOT, "tests", "golden", "persistent_plans.json")) as fh:
        g = json.load(fh)
    assert g["fields"] == FIELDS[7:]
    sw = g["sweep"]
    rows, lines = [], iter(g["index"])
    for k in sw["kernels"]:
        for T in sw["T"]:
            idx = iter(next(lines))
            for G in sw["G"]:
                for nkt in sw["nkt"]:
                    for wt in sw["ws_tiles"]:
                        ws = sw["scratch_floats"] if wt == "scratch_floats" else wt * k["tile_floats"]
                        for sk in sw["streamk"]:
                            rows.append([k["kernel"], T, G, nkt, ws, sk, k["flush"]] + g["plans"][next(idx)])
            assert next(idx, None) is None
    assert next(lines, None) is None
    return rows


def test_sweep_is_the_recorded_one(golden):
    """11 tile counts x 4 grids x 7 k-tile counts x 4 scratch sizes x stream-K on / off, for the 256 x 256 kernel and the
    256 x 128 kernel with flush 0 and 2 -- with rows that decline for each of the two reasons."""
    assert len(golden) == 3 * 11 * 4 * 7 * 4 * 2
    assert {r[1] for r in golden} == {1, 7, 8, 255, 256, 257, 388, 900, 1800, 3600, 65536}
    assert {r[2] for r in golden} == {8, 64, 256, 304}
    assert {r[3] for r in golden} == {2, 4, 8, 16, 17, 32, 64}
    assert {(r[0], r[6]) for r in golden} == {("256x256p", 0), ("256x128p", 0), ("256x128p", 2)}
    assert (48 << 20) in {r[4] for r in golden}
    wp = [r for r in golden if r[0] == "256x256p" and r[14] == "declined"]
    # the scratch: no room for the partial tiles plus the dump tile (here: no scratch at all)
    assert any(r[4] == 0 for r in wp)
    # the plan table: a scratch that holds everything, and still declined
    assert any(r[4] == (48 << 20) and r[1] == 65536 and r[2] == 8 for r in wp)
    assert any(r[0] == "256x128p" and r[14] == "declined" for r in golden)
    assert any(r[0] == "256x128p" and r[14] == "error" for r in golden)
    assert any(r[10] > 0 for r in golden) and any(r[9] > 1 for r in golden)      # both kinds of tail occur


def test_every_field_equals_the_former_launchers(plans, golden):
    _, rows = plans
    assert len(rows) == len(golden)
    for got, want in zip(rows, golden):
        assert [got[f] for f in FIELDS] == want


def test_invariants_of_every_plan_that_fits(plans):
    max_items, rows = plans
    assert max_items == 120
    n = 0
    for r in rows:
        if r["status"] != "fits":
            continue
        n += 1
        T, G = r["T"], r["G"]
        assert r["n_full"] % G == 0, r
        assert r["n_full"] + T % G == T, r
        if r["sk_units"] > 0:      # stream-K: a run of ceil(units / sk_g) units touches at most that many tiles' fragments + 1
            run = -(-r["sk_units"] // r["sk_g"])
            upt = r["nkt"] // r["sk_q"]
            tail_items = (run + upt - 2) // upt + 1
            assert r["n_sp"] == 0 and r["split_p"] == 1, r
        else:
            tail_items = -(-r["n_sp"] // G)
        assert r["n_full"] // G + tail_items <= max_items, r
        assert (r["part_tiles"] + r["dump"]) * r["tile_floats"] <= r["ws_floats"], r
    assert n > 1000
