"""The decisions of the `raft` command line (raft_amd/host/cli_plan.hpp) on the CPU: tests/cli_plan_check.cpp built by the host
compiler under the address and undefined-behaviour sanitizers and run as a process of its own."""
from __future__ import annotations

import shutil

import pytest
from raft_testlib import build_and_run_check


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cli_plan_check(tmp_path):
    build_and_run_check("cli_plan_check", tmp_path)
