"""The rule of include/raft_hip_utg.h as raft_amd/csrc/unitig_rule.hpp states it, on the CPU: tests/unitig_rule_check.cpp built by the
host compiler under the address and undefined-behaviour sanitizers and run as a process of its own -- twin, succ and w, the
consistency rule on one table per violated condition, and a sequential walk on a '+' chain, a mixed-strand chain, the 2-cycle in
both strand forms and a 3-cycle.  The Python walk the GPU tests compare with gives the same layouts on the same tables."""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from unitig_testlib import first_bad_read, make_table, n50, rounds_of, walk

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_unitig_rule_check(tmp_path):
    exe = str(tmp_path / "unitig_rule_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-static-libasan", "-static-libubsan", "-pthread",       # (the runtimes inside the program: nothing to load beside it)
                            os.path.join(HERE, "unitig_rule_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "unitig_rule_check: ok" in run.stdout


def test_the_rule_header_includes_no_hip():
    text = open(os.path.join(HERE, "..", "raft_amd", "csrc", "unitig_rule.hpp")).read()
    assert re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", text) == ["cstdint", "best_ovl_rule.hpp"]
    assert "hip" not in re.sub(r"//.*", "", text).lower().replace("raft_hip", "")


def table(lens, links, skipped=()):
    """The Table of unitig_rule_check.cpp: link = (a, end of a, b, end of b, span)"""
    n = len(lens)
    partner, span, flags = np.full((n, 2), -1, np.int32), np.zeros((n, 2), np.int32), np.zeros(n, np.uint8)
    for a, ea, b, eb, s in links:
        rev = 1 if ea == eb else 0
        for r, e, p in ((a, ea, b), (b, eb, a)):
            partner[r, e], span[r, e] = p, s
            flags[r] |= (2 | rev) << (2 * e)
    flags[list(skipped)] |= 16
    return np.array(lens, np.int32), partner, span, flags


def test_the_python_walk_on_the_tables_of_the_check_program():
    """... with the layouts that program states by hand"""
    w = walk(*table([1000, 400, 600, 800, 50], [(3, 1, 0, 0, 100), (0, 1, 2, 0, 200)], skipped=[4]))
    assert w["unitig"].tolist() == [1, 0, 1, 1, -1] and w["index"].tolist() == [1, 0, 0, 2, -1] and w["orient"].tolist() == [1, 0, 1, 1, 0]
    assert w["offset"].tolist() == [400, 0, 0, 1300, 0] and w["order"].tolist() == [1, 2, 0, 3] and w["utg_off"].tolist() == [0, 1, 4]
    assert w["utg_length"].tolist() == [400, 2100] and w["utg_circular"].tolist() == [0, 0]
    assert w["summary"] == dict(reads_in=5, reads_skipped=1, unitigs=2, singletons=1, circular=0, longest_reads=3, longest_length=2100, total_length=2500)
    w = walk(*table([1000, 2000, 3000, 4000], [(0, 1, 1, 1, 10), (1, 0, 2, 0, 20), (2, 1, 3, 0, 30)]))
    assert w["orient"].tolist() == [0, 1, 0, 0] and w["offset"].tolist() == [0, 990, 2970, 5940] and w["utg_length"].tolist() == [9940]
    w = walk(*table([70, 1000, 3000], [(2, 1, 1, 0, 100), (1, 1, 2, 0, 200)]))
    assert w["unitig"].tolist() == [0, 1, 1] and w["offset"].tolist() == [0, 0, 800] and w["utg_length"].tolist() == [70, 3700] and w["utg_circular"].tolist() == [0, 1]
    w = walk(*table([1000, 3000], [(0, 1, 1, 1, 100), (0, 0, 1, 0, 200)]))
    assert w["orient"].tolist() == [0, 1] and w["offset"].tolist() == [0, 900] and w["utg_length"].tolist() == [3700] and w["utg_circular"].tolist() == [1]
    w = walk(*table([-4, 1000, 2000, 3000], [(1, 1, 3, 1, 10), (3, 0, 2, 0, 20), (2, 1, 1, 0, 30)]))
    assert w["index"].tolist() == [0, 0, 2, 1] and w["orient"].tolist() == [0, 0, 0, 1] and w["offset"].tolist() == [0, 0, 3970, 990]
    assert w["order"].tolist() == [0, 1, 3, 2] and w["utg_length"].tolist() == [0, 5940] and w["utg_circular"].tolist() == [0, 1]
    assert w["summary"]["circular"] == 1 and w["summary"]["total_length"] == 5940 and w["summary"]["longest_reads"] == 3


def test_the_generator_makes_what_it_is_asked_for():
    rng = np.random.default_rng(0)
    L, partner, span, flags = make_table(rng, 500, [(100, False), (64, True), (1, False), (2, True), (2, False)], skipped=30)
    assert first_bad_read(L, partner, span, flags) == -1
    w = walk(L, partner, span, flags)
    s = w["summary"]
    assert (s["reads_skipped"], s["circular"], s["longest_reads"], s["unitigs"]) == (30, 2, 100, 4 + (500 - 169 - 30) + 1)
    assert sorted(w["utg_reads"][w["utg_circular"] == 1].tolist()) == [2, 64]
    assert np.array_equal(np.sort(w["order"]), np.flatnonzero((flags & 16) == 0)) and np.array_equal(np.diff(w["utg_off"]), w["utg_reads"])
    assert np.array_equal(w["order"][w["utg_off"][:-1]], np.sort(w["order"][w["utg_off"][:-1]]))          # ids in the order of the start reads
    assert [rounds_of(n) for n in (0, 1, 2, 3, 4, 5, 1024, 1025)] == [0, 1, 2, 3, 3, 4, 11, 12]
    assert [n50(x) for x in ([], [7], [5, 5, 5, 5], [10, 6, 4], [10, 6, 5], [2 ** 40, 2 ** 40, 3])] == [0, 7, 5, 10, 6, 2 ** 40]
