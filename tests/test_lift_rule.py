"""The rule of include/raft_hip_lift.h as raft_amd/csrc/lift_rule.hpp states it, on the CPU: tests/lift_rule_check.cpp built by the
host compiler under the address and undefined-behaviour sanitizers and run as a process of its own -- fixed cases, the rule's
properties (outputs inside their rows and sides, mirror images, the identity table) on random tables with overlapping rows, spans
near 2^31 - 1 on both sides.  The Python oracle the GPU tests compare with gives the same outputs on the same fixed cases and holds
the same properties."""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from lift_testlib import as_multiset, identity_table, lift, lift_record, make_stream, make_table, mirror

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_lift_rule_check(tmp_path):
    exe = str(tmp_path / "lift_rule_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-static-libasan", "-static-libubsan", "-pthread",       # (the runtimes inside the program: nothing to load beside it)
                            os.path.join(HERE, "lift_rule_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "lift_rule_check: ok" in run.stdout


def test_the_rule_header_includes_no_hip():
    text = open(os.path.join(HERE, "..", "raft_amd", "csrc", "lift_rule.hpp")).read()
    assert re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", text) == ["cstdint"]
    assert "hip" not in re.sub(r"//.*", "", text).lower().replace("raft_hip", "").replace("__hipcc__", "")


OFF, FB, FE = [0, 1, 3, 3], [0, 0, 500], [1000, 600, 1200]


def test_the_python_oracle_on_the_fixed_cases_of_the_check_program():
    """... with the outputs that program states by hand"""
    def one(rec, min_len=1):
        return lift_record(OFF, FB, FE, rec, min_len)
    assert one((0, 0, 100, 0, 200, 300, 0)) == ([], 0) and one((0, 100, 100, 1, 0, 100, 0)) == ([], 0) and one((0, 0, 100, 2, 0, 100, 0)) == ([], 0)
    assert one((0, 100, 400, 1, 50, 350, 0))[0] == [(0, 100, 400, 1, 50, 350)]
    assert one((0, 100, 400, 1, 620, 920, 1))[0] == [(0, 100, 400, 2, 120, 420)]
    assert one((0, 0, 400, 1, 400, 800, 0))[0] == [(0, 0, 200, 1, 400, 600), (0, 100, 400, 2, 0, 300)]
    assert one((0, 0, 400, 1, 400, 800, 1))[0] == [(0, 200, 400, 1, 400, 600), (0, 0, 300, 2, 0, 300)]
    assert one((1, 400, 800, 0, 0, 400, 0))[0] == [(1, 400, 600, 0, 0, 200), (2, 0, 300, 0, 100, 400)]
    assert one((0, -50, 1100, 1, 100, 1250, 0))[0] == [(0, 0, 450, 1, 150, 600), (0, 350, 1000, 2, 0, 650)]
    assert one((0, 100, 300, 1, 400, 800, 0))[0] == [(0, 100, 200, 1, 400, 600), (0, 150, 300, 2, 0, 300)]
    assert one((0, 0, 400, 1, 400, 800, 0), 200)[1] == 0 and one((0, 0, 400, 1, 400, 800, 0), 201) == ([(0, 100, 400, 2, 0, 300)], 1)
    assert one((0, 0, 400, 1, 400, 800, 0), 301) == ([], 2)
    assert one((0, 0, 400, 1, 0, 100, 0), 101) == ([], 1) and one((0, 0, 400, 1, 0, 100, 0), 100) == ([(0, 0, 400, 1, 0, 100)], 0)


def test_the_python_oracle_holds_the_properties():
    rng = np.random.default_rng(3)
    read_len, off, fb, fe = make_table(rng, 30, rows_choice=(0, 1, 2, 3, 6))
    cols, strand = make_stream(rng, read_len, 3000)
    for min_len in (1, 2, 501):
        a = lift(off, fb, fe, cols, strand, min_len)
        b = lift(off, fb, fe, *mirror(cols, strand), min_len)
        assert as_multiset(a) == as_multiset(b, mirrored=True) and a["pairs_dropped"] == b["pairs_dropped"]
        for side in ("q", "t"):
            row, s, e = a[side + "frag"], a[side + "s"].astype(np.int64), a[side + "e"].astype(np.int64)
            assert np.all((0 <= s) & (e - s >= min_len) & (e <= fe[row].astype(np.int64) - fb[row]))
        assert np.all(np.diff(a["src"]) >= 0) and a["n_out"] == a["src"].size
        assert a["records_none"] + np.unique(a["src"]).size == a["n_records"]
    # one row [0, len) per read: every in-range record that is not a read with itself lifts to itself
    ioff, ifb, ife = identity_table(read_len)
    inside = (cols[1] >= 0) & (cols[2] <= read_len[cols[0]]) & (cols[4] >= 0) & (cols[5] <= read_len[cols[3]])
    keep = inside & (cols[0] != cols[3]) & (cols[2] > cols[1]) & (cols[5] > cols[4])
    assert keep.sum() > 500
    got = lift(ioff, ifb, ife, [c[inside] for c in cols], strand[inside])
    want = [c[keep] for c in cols]
    assert all(np.array_equal(got[k], w) for k, w in zip(("qfrag", "qs", "qe", "tfrag", "ts", "te"), want))
    assert np.array_equal(got["rev"], strand[keep]) and got["records_cut"] == 0 and got["most_per_record"] == 1
