"""The rule of include/raft_hip_best.h as raft_amd/csrc/best_ovl_rule.hpp states it, on the CPU: tests/best_ovl_rule_check.cpp built by
the host compiler under the address and undefined-behaviour sanitizers and run as a process of its own -- the key's round trips and
its order, the partner end, and over every record between reads of lengths 1..5 that a set counted on both sides gives the table of
the mirrored set counted on its query sides, in any order, and that mutuality is symmetric."""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_best_ovl_rule_check(tmp_path):
    exe = str(tmp_path / "best_ovl_rule_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-static-libasan", "-static-libubsan", "-pthread",       # (the runtimes inside the program: nothing to load beside it)
                            os.path.join(HERE, "best_ovl_rule_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "best_ovl_rule_check: ok" in run.stdout


def test_the_rule_header_includes_no_hip():
    text = open(os.path.join(HERE, "..", "raft_amd", "csrc", "best_ovl_rule.hpp")).read()
    assert re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", text) == ["cstdint", "ovl_ends_rule.hpp"]
    assert "hip" not in re.sub(r"//.*", "", text).lower().replace("raft_hip", "")
