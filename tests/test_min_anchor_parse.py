"""The argument of `raft --repeat-overlaps A` (raft_cli::parse_min_anchor, raft_amd/host/cli_plan.hpp) on the CPU: tests/min_anchor_check.cpp
built by the host compiler under the address and undefined-behaviour sanitizers and run as a process of its own."""
from __future__ import annotations

import shutil

import pytest
from raft_testlib import build_and_run_check


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_min_anchor_check(tmp_path):
    build_and_run_check("min_anchor_check", tmp_path)
