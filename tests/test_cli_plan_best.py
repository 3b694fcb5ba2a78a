"""What `raft --best-overlaps` adds to raft_amd/host/cli_plan.hpp, on the CPU: tests/cli_plan_best_check.cpp built by the host compiler
under the address and undefined-behaviour sanitizers and run as a process of its own -- that the option needs --overlap-ends, and the
text of the stdout line."""
from __future__ import annotations

import shutil

import pytest
from raft_testlib import build_and_run_check


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cli_plan_best_check(tmp_path):
    build_and_run_check("cli_plan_best_check", tmp_path)
