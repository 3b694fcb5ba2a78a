"""What `raft --graph-clean` adds to raft_amd/host/cli_plan.hpp, on the CPU: tests/cli_plan_graph_clean_check.cpp built by the host
compiler under the address and undefined-behaviour sanitizers and run as a process of its own -- the four new rows in the open table,
the parsers at their bounds, that the option needs --string-graph and its values need the option, that it asks nothing new of the job,
and the two stdout lines.  The usage errors through the program itself: they are decided before any device is looked for."""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import pytest
from raft_testlib import ROOT, build_and_run_check

HERE = os.path.dirname(os.path.abspath(__file__))
RAFT = os.path.join(HERE, "..", "raft_amd", "bin", "raft")
GRAPH = ["--overlap-ends", "100", "--string-graph"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_cli_plan_graph_clean_check(tmp_path):
    build_and_run_check("cli_plan_graph_clean_check", tmp_path)


def test_the_rows_are_in_the_open_tables():
    plan = open(os.path.join(ROOT, "raft_amd", "host", "cli_plan.hpp")).read()
    table = re.search(r"inline constexpr LongOption kOpenLongOptions\[\] = \{(.*?)^\};", plan, flags=re.S | re.M).group(1)
    names = re.findall(r'^\s*\{"([a-z-]+)",', table, flags=re.M)
    assert all(n in names for n in ("graph-clean", "clean-min-ratio", "clean-tip-reads", "clean-rounds"))
    main = open(os.path.join(ROOT, "raft_amd", "host", "raft_main.cpp")).read()
    assert "kOpenLongOptions" in main and "every_long_option_count()" in main
    rows = re.findall(r'^    \{"(\w+)", \[\]\(const Job &j\)', main, flags=re.M)
    assert rows.index("fragment_paf") < rows.index("graph_clean") < rows.index("graph_clean_unitigs")
    assert re.search(r'\{"graph_clean", \[\]\(const Job &j\) \{ return j\.p\.graph_clean; \}, Stage::stream,', main)


@pytest.mark.parametrize("args", [["--graph-clean"], ["--overlap-ends", "100", "--graph-clean"], GRAPH + ["--clean-min-ratio", "400"],
                                  GRAPH + ["--clean-tip-reads", "2"], GRAPH + ["--clean-rounds", "2"], GRAPH + ["--graph-clean", "--clean-rounds", "0"],
                                  GRAPH + ["--graph-clean", "--clean-rounds", "65"], GRAPH + ["--graph-clean", "--clean-min-ratio", "1001"],
                                  GRAPH + ["--graph-clean", "--clean-tip-reads", "-1"], GRAPH + ["--graph-clean=1"]],
                         ids=["without --string-graph", "with --overlap-ends alone", "--clean-min-ratio without the option", "--clean-tip-reads without the option",
                              "--clean-rounds without the option", "no round", "65 rounds", "a ratio above 1000", "a negative T", "an argument to the flag"])
def test_usage_errors(tmp_path, args):
    """The usage and exit code 1, before any input is opened and any device looked for, with nothing written."""
    run = subprocess.run([RAFT, "-e", "30", "-o", str(tmp_path / "out")] + args + [str(tmp_path / "none.fa"), str(tmp_path / "none.paf")],
                         capture_output=True, text=True, cwd=tmp_path)
    assert run.returncode == 1 and "Usage: raft [options] <input-reads.fa> <in.paf>" in run.stdout
    assert "ERROR" not in run.stdout and list(tmp_path.iterdir()) == []


@pytest.mark.parametrize("more", [[], ["--clean-min-ratio", "0", "--clean-tip-reads", "2147483647", "--clean-rounds", "64"],
                                  ["--clean-min-ratio", "1000", "--clean-tip-reads", "0", "--clean-rounds", "1", "--components", "--best-overlaps", "--unitigs",
                                   "--containment", "--fragment-paf"]])
def test_the_options_are_known(tmp_path, more):
    """With --string-graph the command line is accepted: the program goes on to its inputs, which are not there."""
    run = subprocess.run([RAFT, "-e", "30", "-o", str(tmp_path / "out")] + GRAPH + ["--graph-clean"] + more +
                         [str(tmp_path / "none.fa"), str(tmp_path / "none.paf")], capture_output=True, text=True, cwd=tmp_path)
    assert "Usage: raft" not in run.stdout and "unrecognized option" not in run.stderr
    assert "INFO, printParams(), reso = 50" in run.stdout
