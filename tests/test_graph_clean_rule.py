"""The rule of include/raft_hip_cln.h as raft_amd/csrc/graph_clean_rule.hpp states it, on the CPU: tests/graph_clean_rule_check.cpp built
by the host compiler under the address and undefined-behaviour sanitizers and run as a process of its own -- the weak predicate at
equality, one span unit below it and at the edge of the 64-bit products, the candidate predicate at reads == T and T + 1 and with
T = 0, "beats" as a strict total order among candidates, and what makes an edge bad.  And that the rule stands once: the rule header
includes no HIP, the kernels call its functions, and the public header states the rule, the invariant and both departures."""
from __future__ import annotations

import os
import re
import shutil

import pytest
from raft_testlib import ROOT, build_and_run_check


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_graph_clean_rule_check(tmp_path):
    build_and_run_check("graph_clean_rule_check", tmp_path)


def test_the_rule_header_includes_no_hip():
    text = open(os.path.join(ROOT, "raft_amd", "csrc", "graph_clean_rule.hpp")).read()
    includes = re.findall(r'^#include\s+[<"]([^>"]+)[>"]', text, flags=re.M)
    assert includes == ["cstdint", "unitig_rule.hpp"]
    assert "hip_runtime" not in text and "__global__" not in text and "__device__" not in text
    # ... and the kernels take the rule from it: no second statement of a predicate
    kernels = open(os.path.join(ROOT, "raft_amd", "csrc", "graph_clean.hpp")).read()
    assert '#include "graph_clean_rule.hpp"' in kernels
    for fn in ("cln_edge_ok", "cln_weak", "cln_candidate", "cln_beats", "cln_isolated_short"):
        assert re.search(r"\b%s\(" % fn, kernels), fn
    code = re.sub(r"//.*", "", kernels)
    assert "* 1000" not in code and "1000 *" not in code and ".length >" not in code and ".first <" not in code


def test_the_public_header_states_the_rule_the_invariant_and_both_departures():
    text = re.sub(r"\s*\n \* ", " ", open(os.path.join(ROOT, "include", "raft_hip_cln.h")).read())
    for phrase in ("span * 1000 < W * m(u)", "products taken in 64 bits", "u >> 1 == w >> 1", "also stands at a smaller index", "deg(u) == 1",
                   "(reads, length, -first)", "strict total order", "x != b", "as the round found it", "The invariant:",
                   "w keeps at least one live arc after that round", "asg_cut_tip deletes as it walks", "dead at both ends", "asg_arc_del_short",
                   "consistency check by construction", "T = 0 makes no chain a candidate", "W = 0 cuts nothing"):
        assert phrase in text, phrase
