"""The rule of include/raft_hip_ctn.h as raft_amd/csrc/containment_rule.hpp states it, on the CPU: tests/containment_rule_check.cpp built by
the host compiler under the address and undefined-behaviour sanitizers and run as a process of its own -- acceptability at equal
lengths and ids, both views, the clamp on either side, the order of the keys at each tie, the composition over all strand pairs."""
from __future__ import annotations

import os
import re
import shutil

import pytest
from raft_testlib import ROOT, build_and_run_check


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_containment_rule_check(tmp_path):
    build_and_run_check("containment_rule_check", tmp_path)


def test_the_rule_header_includes_no_hip():
    text = open(os.path.join(ROOT, "raft_amd", "csrc", "containment_rule.hpp")).read()
    assert re.findall(r'^#include\s+[<"]([^>"]+)[>"]', text, flags=re.M) == ["ovl_ends_rule.hpp"]
    assert "hip_runtime" not in text and "__global__" not in text and "__device__" not in text
    # ... and the kernels take the rule from it: no second statement of the keys, the clamp or the composition
    kernels = open(os.path.join(ROOT, "raft_amd", "csrc", "containment.hpp")).read()
    assert '#include "containment_rule.hpp"' in kernels
    for fn in ("ctn_query_view", "ctn_target_view", "ctn_acceptable", "ctn_key1", "ctn_key1_parent", "ctn_view_key2", "ctn_key2_pos", "ctn_compose",
               "ctn_unitig_start", "ctn_depth_permille"):
        assert re.search(r"\b%s\(" % fn, kernels), fn
    assert "<< 31" not in kernels and "<< 32" not in kernels and "0x7FFFFFFF" not in kernels


def test_the_public_header_states_the_rule():
    text = open(os.path.join(ROOT, "include", "raft_hip_ctn.h")).read()
    for phrase in ("lc > lr or (lc == lr and c < r)", "key1 = (uint64)lc << 31 | (uint64)(0x7FFFFFFF - c)", "pos_raw = rev ? bs - (lr - ae) : bs - as",
                   "pos = min(max(pos_raw, 0), lc - lr)", "key2 = (uint64)span << 32 | (uint64)rev << 31 | (uint64)(0x7FFFFFFF - pos)",
                   "root_pos(r) = V ? P + (len[a] - p - lr) : P + p", "NO WRAP on circular unitigs", "placed_bases * 1000 / length"):
        assert phrase in text, phrase
