"""CPU: `raft --fragment-overlaps` takes no argument: `--fragment-overlaps=3` is rejected the way any bad option is -- the usage text on
stdout, exit code 1, before any device is asked for --, and the plain option passes the parser: the run gets as far as the device (where
there is none, the engine's device error is its last line; where there is one, the job runs and the option's line is the last)."""
import os
import subprocess

from raft_testlib import ROOT
from test_cli_early_exits import PAF, READS, USAGE

RAFT = os.path.join(ROOT, "raft_amd", "bin", "raft")


def run(tmp_path, *options):
    (tmp_path / "a.fa").write_text(READS)
    (tmp_path / "b.paf").write_text(PAF)
    return subprocess.run([RAFT, "-e", "30", *options, "a.fa", "b.paf"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def test_an_argument_prints_the_usage(tmp_path):
    r = run(tmp_path, "--fragment-overlaps=3")
    assert r.returncode == 1, r.stdout.decode() + r.stderr.decode()
    assert r.stdout.decode() == USAGE
    assert sorted(os.listdir(tmp_path)) == ["a.fa", "b.paf"]          # (not even the output FASTA is created)


def test_the_plain_option_reaches_the_device(tmp_path):
    r = run(tmp_path, "--fragment-overlaps")
    out = r.stdout.decode()
    assert "Usage:" not in out and out.startswith("INFO, printParams(), reso = 50\n")
    lines = out.split("\n")
    if r.returncode == 0:
        assert lines[-2].startswith("INFO, fragment_overlaps(), fragments = ") and os.path.exists(tmp_path / "raft.fragments.tsv")
    else:
        assert r.returncode == 1 and lines[-2].startswith("ERROR, raft_hip_create(), device 0: "), out
        assert not os.path.exists(tmp_path / "raft.fragments.tsv")
