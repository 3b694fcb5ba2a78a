"""What `raft --components` adds to raft_amd/host/cli_plan.hpp, on the CPU: tests/cli_plan_components_check.cpp built by the host
compiler under the address and undefined-behaviour sanitizers and run as a process of its own -- the new row through long_option, the
thirteen rows before it unchanged, that the option needs --overlap-ends, that it asks nothing new of the job, and the stdout line.  The
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
def test_cli_plan_components_check(tmp_path):
    build_and_run_check("cli_plan_components_check", tmp_path)


@pytest.mark.parametrize("args", [["--components"], ["--components", "--best-overlaps"], ["--components", "--ends-min-ratio", "900"],
                                  ["--overlap-ends", "100", "--components=1"], ["--overlap-ends", "x", "--components"]],
                         ids=["without --overlap-ends", "beside another option that needs it", "beside the ratio alone", "an argument to the flag",
                              "an --overlap-ends that is no number"])
def test_usage_errors(tmp_path, args):
    """The usage and exit code 1, before any input is opened and any device looked for."""
    run = subprocess.run([RAFT, "-e", "30", "-o", str(tmp_path / "out")] + args + [str(tmp_path / "none.fa"), str(tmp_path / "none.paf")],
                         capture_output=True, text=True, cwd=tmp_path)
    assert run.returncode == 1 and "Usage: raft [options] <input-reads.fa> <in.paf>" in run.stdout
    assert "ERROR" not in run.stdout and list(tmp_path.iterdir()) == []


def test_the_option_is_known(tmp_path):
    """With --overlap-ends the command line is accepted: the program goes on to its inputs, which are not there."""
    run = subprocess.run([RAFT, "-e", "30", "-o", str(tmp_path / "out"), "--overlap-ends", "100", "--components", str(tmp_path / "none.fa"),
                          str(tmp_path / "none.paf")], capture_output=True, text=True, cwd=tmp_path)
    assert "Usage: raft" not in run.stdout and "unrecognized option" not in run.stderr
    assert "INFO, printParams(), reso = 50" in run.stdout
