"""The argument of `raft --repeat-overlaps A` (raft_cli::parse_min_anchor, raft_amd/host/cli_plan.hpp) on the CPU: tests/min_anchor_check.cpp
built by the host compiler under the address and undefined-behaviour sanitizers and run as a process of its own."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_min_anchor_check(tmp_path):
    exe = str(tmp_path / "min_anchor_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-static-libasan", "-static-libubsan", "-pthread",       # (the runtimes inside the program: nothing to load beside it)
                            os.path.join(HERE, "min_anchor_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "min_anchor_check: ok" in run.stdout
