"""What `raft --containment` adds to raft_amd/host/cli_plan.hpp, on the CPU: tests/cli_plan_containment_check.cpp built by the host compiler
under the address and undefined-behaviour sanitizers and run as a process of its own -- the new row in a fourth table, the sixteen rows
before it unchanged under long_option and any_long_option, one list of tables walked end to end, that the option needs --overlap-ends,
that it asks nothing new of the job, and the two stdout lines.  The usage errors through the program itself: they are decided before
any device is looked for."""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import pytest
from raft_testlib import ROOT, build_and_run_check

HERE = os.path.dirname(os.path.abspath(__file__))
RAFT = os.path.join(HERE, "..", "raft_amd", "bin", "raft")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cli_plan_containment_check(tmp_path):
    build_and_run_check("cli_plan_containment_check", tmp_path)


def test_the_command_line_walks_the_one_list():
    main = open(os.path.join(ROOT, "raft_amd", "host", "raft_main.cpp")).read()
    assert "every_long_option_count()" in main and main.count("every_long_option(") >= 3 and "any_long_option" not in main
    rows = re.findall(r'^    \{"(\w+)", \[\]\(const Job &j\)', main, flags=re.M)
    at = rows.index("string_graph")
    assert rows[at:at + 4] == ["string_graph", "containment", "place_contained", "fragment_paf"]
    assert re.search(r'\{"containment", \[\]\(const Job &j\) \{ return j\.p\.containment; \}, Stage::stream,', main)
    assert re.search(r'\{"place_contained", \[\]\(const Job &j\) \{ return j\.p\.containment && j\.p\.unitigs; \}, Stage::stream,', main)


@pytest.mark.parametrize("args", [["--containment"], ["--containment", "--best-overlaps"], ["--overlap-ends", "100", "--containment=1"],
                                  ["--overlap-ends", "100", "--containment", "--unitigs"]],
                         ids=["without --overlap-ends", "beside an option that lacks it too", "an argument to the flag", "--unitigs without --best-overlaps"])
def test_usage_errors(tmp_path, args):
    """The usage and exit code 1, before any input is opened and any device looked for."""
    run = subprocess.run([RAFT, "-e", "30", "-o", str(tmp_path / "out")] + args + [str(tmp_path / "none.fa"), str(tmp_path / "none.paf")],
                         capture_output=True, text=True, cwd=tmp_path)
    assert run.returncode == 1 and "Usage: raft [options] <input-reads.fa> <in.paf>" in run.stdout
    assert "ERROR" not in run.stdout and list(tmp_path.iterdir()) == []


@pytest.mark.parametrize("more", [[], ["--best-overlaps", "--unitigs"], ["--string-graph", "--components", "--best-overlaps", "--unitigs", "--fragment-paf"]])
def test_the_option_is_known(tmp_path, more):
    """With --overlap-ends the command line is accepted: the program goes on to its inputs, which are not there."""
    run = subprocess.run([RAFT, "-e", "30", "-o", str(tmp_path / "out"), "--overlap-ends", "100", "--containment"] + more +
                         [str(tmp_path / "none.fa"), str(tmp_path / "none.paf")], capture_output=True, text=True, cwd=tmp_path)
    assert "Usage: raft" not in run.stdout and "unrecognized option" not in run.stderr
    assert "INFO, printParams(), reso = 50" in run.stdout
