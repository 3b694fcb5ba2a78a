"""What `raft --fragment-paf / --fragment-paf-min` adds to raft_amd/host/cli_plan.hpp, on the CPU: tests/cli_plan_lift_check.cpp built
by the host compiler under the address and undefined-behaviour sanitizers and run as a process of its own -- the text of L, that it
needs --fragment-paf, the column mask that asks for the strand, the query ids kept past prepare_input, and the stdout line.  The
usage errors through the program itself: they are decided before any device is looked for."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest
from raft_testlib import build_and_run_check

HERE = os.path.dirname(os.path.abspath(__file__))
RAFT = os.path.join(HERE, "..", "raft_amd", "bin", "raft")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cli_plan_lift_check(tmp_path):
    build_and_run_check("cli_plan_lift_check", tmp_path)


@pytest.mark.parametrize("args", [["--fragment-paf-min", "5"], ["--fragment-paf", "--fragment-paf-min", "0"], ["--fragment-paf", "--fragment-paf-min", "x"],
                                  ["--fragment-paf", "--fragment-paf-min"], ["--fragment-paf=1"], ["--fragment-paf", "--fragment-paf-min", "-1"]],
                         ids=["min without the option", "min 0", "min not a number", "min without a value", "an argument to the flag", "min negative"])
def test_usage_errors(tmp_path, args):
    """The usage and exit code 1, before any input is opened and any device looked for."""
    run = subprocess.run([RAFT, "-e", "30", "-o", str(tmp_path / "out")] + args + [str(tmp_path / "none.fa"), str(tmp_path / "none.paf")],
                         capture_output=True, text=True, cwd=tmp_path)
    assert run.returncode == 1 and "Usage: raft [options] <input-reads.fa> <in.paf>" in run.stdout
    assert "ERROR" not in run.stdout and not os.path.exists(tmp_path / "out.reads.fasta")
