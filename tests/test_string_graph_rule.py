"""The rule of include/raft_hip_sg.h as raft_amd/csrc/string_graph_rule.hpp states it, on the CPU: tests/string_graph_rule_check.cpp built
by the host compiler under the address and undefined-behaviour sanitizers and run as a process of its own -- over every record between
reads of lengths 1..6 on both strands that a dovetail view gives an arc with ext >= 1 and back >= 1, that a record's two views give
twin arcs with one key, the key's order, and the reducible predicate at the fuzz, one beyond it and at a tie in ext."""
from __future__ import annotations

import os
import re
import shutil

import pytest
from raft_testlib import ROOT, build_and_run_check


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_string_graph_rule_check(tmp_path):
    build_and_run_check("string_graph_rule_check", tmp_path)


def test_the_rule_header_includes_no_hip():
    text = open(os.path.join(ROOT, "raft_amd", "csrc", "string_graph_rule.hpp")).read()
    includes = re.findall(r'^#include\s+[<"]([^>"]+)[>"]', text, flags=re.M)
    assert includes == ["cstdint", "best_ovl_rule.hpp"]
    assert "hip_runtime" not in text and "__global__" not in text and "__device__" not in text
    # ... and the kernels take the rule from it: no second statement of ext, back or the predicate
    kernels = open(os.path.join(ROOT, "raft_amd", "csrc", "string_graph.hpp")).read()
    assert '#include "string_graph_rule.hpp"' in kernels
    for fn in ("sg_view_arc", "sg_key", "sg_key_wins", "sg_reducible"):
        assert re.search(r"\b%s\(" % fn, kernels), fn
    assert "t3 - q3" not in kernels and "t5 - q5" not in kernels


def test_the_public_header_states_the_rule_and_the_departure():
    text = open(os.path.join(ROOT, "include", "raft_hip_sg.h")).read()
    for phrase in ("ext = t3 - q3", "back = q5 - t5", "ext = t5 - q5", "back = q3 - t3", "(span, -ext_lo, -ext_hi)", "asg_arc_del_trans", "departs",
                   "consistency check by construction"):
        assert phrase in text, phrase
