"""The rule of include/raft_hip_end.h as raft_amd/csrc/ovl_ends_rule.hpp states it, on the CPU: tests/ovl_ends_rule_check.cpp built by
the host compiler under the address and undefined-behaviour sanitizers and run as a process of its own -- the mirror property over
every record of lengths 1..6, a table of cases worked out by hand, 64-bit safety near INT32_MAX."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_ovl_ends_rule_check(tmp_path):
    exe = str(tmp_path / "ovl_ends_rule_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-static-libasan", "-static-libubsan", "-pthread",       # (the runtimes inside the program: nothing to load beside it)
                            os.path.join(HERE, "ovl_ends_rule_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ovl_ends_rule_check: ok" in run.stdout
