"""What `raft --unitigs` adds to raft_amd/host/cli_plan.hpp, on the CPU: tests/cli_plan_unitigs_check.cpp built by the host compiler
under the address and undefined-behaviour sanitizers and run as a process of its own -- that the option needs --best-overlaps, the
N50 (no unitigs, one, ties, the exact half, totals beyond 2^32) and the text of the stdout line."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cli_plan_unitigs_check(tmp_path):
    exe = str(tmp_path / "cli_plan_unitigs_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-static-libasan", "-static-libubsan", "-pthread",       # (the runtimes inside the program: nothing to load beside it)
                            os.path.join(HERE, "cli_plan_unitigs_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "cli_plan_unitigs_check: ok" in run.stdout
