"""What `raft --fragment-paf / --fragment-paf-min` adds to raft_amd/host/cli_plan.hpp, on the CPU: tests/cli_plan_lift_check.cpp built
by the host compiler under the address and undefined-behaviour sanitizers and run as a process of its own -- the text of L, that it
needs --fragment-paf, the column mask that asks for the strand, the query ids kept past prepare_input, and the stdout line.  The
usage errors through the program itself: they are decided before any device is looked for."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
RAFT = os.path.join(HERE, "..", "raft_amd", "bin", "raft")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cli_plan_lift_check(tmp_path):
    exe = str(tmp_path / "cli_plan_lift_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-static-libasan", "-static-libubsan", "-pthread",       # (the runtimes inside the program: nothing to load beside it)
                            os.path.join(HERE, "cli_plan_lift_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "cli_plan_lift_check: ok" in run.stdout


@pytest.mark.parametrize("args", [["--fragment-paf-min", "5"], ["--fragment-paf", "--fragment-paf-min", "0"], ["--fragment-paf", "--fragment-paf-min", "x"],
                                  ["--fragment-paf", "--fragment-paf-min"], ["--fragment-paf=1"], ["--fragment-paf", "--fragment-paf-min", "-1"]],
                         ids=["min without the option", "min 0", "min not a number", "min without a value", "an argument to the flag", "min negative"])
def test_usage_errors(tmp_path, args):
    """The usage and exit code 1, before any input is opened and any device looked for."""
    run = subprocess.run([RAFT, "-e", "30", "-o", str(tmp_path / "out")] + args + [str(tmp_path / "none.fa"), str(tmp_path / "none.paf")],
                         capture_output=True, text=True, cwd=tmp_path)
    assert run.returncode == 1 and "Usage: raft [options] <input-reads.fa> <in.paf>" in run.stdout
    assert "ERROR" not in run.stdout and not os.path.exists(tmp_path / "out.reads.fasta")
