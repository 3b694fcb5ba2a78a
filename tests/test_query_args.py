"""The argument decisions of the record-stream queries (raft_amd/csrc/query_args.hpp: which columns must be there, what the three
arrays of a CSR table say, which load path the columns allow) on the CPU: tests/query_args_check.cpp built by the host compiler
under the address and undefined-behaviour sanitizers and run as a process of its own."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_query_args_check(tmp_path):
    exe = str(tmp_path / "query_args_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-static-libasan", "-static-libubsan",       # (the runtimes inside the program: nothing to load beside it)
                            os.path.join(HERE, "query_args_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "query_args_check: ok" in run.stdout
