"""What `raft --string-graph` adds to raft_amd/host/cli_plan.hpp, on the CPU: tests/cli_plan_string_graph_check.cpp built by the host
compiler under the address and undefined-behaviour sanitizers and run as a process of its own -- the two new rows in a third table, the
fourteen rows before them unchanged under long_option, that the option needs --overlap-ends and the fuzz the option, that it asks
nothing new of the job, and the stdout line.  The usage errors through the program itself: they are decided before any device is
looked for."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest
from raft_testlib import build_and_run_check

HERE = os.path.dirname(os.path.abspath(__file__))
RAFT = os.path.join(HERE, "..", "raft_amd", "bin", "raft")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cli_plan_string_graph_check(tmp_path):
    build_and_run_check("cli_plan_string_graph_check", tmp_path)


@pytest.mark.parametrize("args", [["--string-graph"], ["--string-graph", "--string-graph-fuzz", "10"], ["--overlap-ends", "100", "--string-graph-fuzz", "10"],
                                  ["--string-graph-fuzz", "10"], ["--overlap-ends", "100", "--string-graph=1"],
                                  ["--overlap-ends", "100", "--string-graph", "--string-graph-fuzz", "-1"],
                                  ["--overlap-ends", "100", "--string-graph", "--string-graph-fuzz", "2147483648"],
                                  ["--overlap-ends", "100", "--string-graph", "--string-graph-fuzz"]],
                         ids=["without --overlap-ends", "with its fuzz, without --overlap-ends", "the fuzz without the option", "the fuzz alone",
                              "an argument to the flag", "a negative fuzz", "a fuzz beyond int32", "a fuzz without its number"])
def test_usage_errors(tmp_path, args):
    """The usage and exit code 1, before any input is opened and any device looked for."""
    run = subprocess.run([RAFT, "-e", "30", "-o", str(tmp_path / "out")] + args + [str(tmp_path / "none.fa"), str(tmp_path / "none.paf")],
                         capture_output=True, text=True, cwd=tmp_path)
    assert run.returncode == 1 and "Usage: raft [options] <input-reads.fa> <in.paf>" in run.stdout
    assert "ERROR" not in run.stdout and list(tmp_path.iterdir()) == []


@pytest.mark.parametrize("more", [[], ["--string-graph-fuzz", "0"], ["--string-graph-fuzz", "2147483647", "--components", "--best-overlaps", "--unitigs"]])
def test_the_options_are_known(tmp_path, more):
    """With --overlap-ends the command line is accepted: the program goes on to its inputs, which are not there."""
    run = subprocess.run([RAFT, "-e", "30", "-o", str(tmp_path / "out"), "--overlap-ends", "100", "--string-graph"] + more +
                         [str(tmp_path / "none.fa"), str(tmp_path / "none.paf")], capture_output=True, text=True, cwd=tmp_path)
    assert "Usage: raft" not in run.stdout and "unrecognized option" not in run.stderr
    assert "INFO, printParams(), reso = 50" in run.stdout
