"""What `raft --overlap-ends / --ends-min-ratio` adds to raft_amd/host/cli_plan.hpp, on the CPU: tests/cli_plan_ends_check.cpp built by
the host compiler under the address and undefined-behaviour sanitizers and run as a process of its own -- which texts the two options
take, that the second needs the first, the tokeniser's column mask and the text of the stdout line."""
from __future__ import annotations

import shutil

import pytest
from raft_testlib import build_and_run_check


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cli_plan_ends_check(tmp_path):
    build_and_run_check("cli_plan_ends_check", tmp_path)
