"""CPU: `raft --repeat-overlaps A` rejects an A that is not a whole number from 1 to INT32_MAX the way it rejects any bad option -- the
usage text on stdout, exit code 1, before any device is asked for -- and the usage text itself is what it was."""
import os
import subprocess

import pytest
from raft_testlib import ROOT
from test_cli_early_exits import PAF, READS, USAGE

RAFT = os.path.join(ROOT, "raft_amd", "bin", "raft")


@pytest.mark.parametrize("value", ["0", "-1", "x", "", "1.5", "3x", " 4", "+2", "2147483648", "99999999999999999999"])
def test_a_bad_min_anchor_prints_the_usage(tmp_path, value):
    (tmp_path / "a.fa").write_text(READS)
    (tmp_path / "b.paf").write_text(PAF)
    r = subprocess.run([RAFT, "-e", "30", "--repeat-overlaps", value, "a.fa", "b.paf"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1, r.stdout.decode() + r.stderr.decode()
    assert r.stdout.decode() == USAGE
    assert sorted(os.listdir(tmp_path)) == ["a.fa", "b.paf"]          # (not even the output FASTA is created)


def test_repeat_overlaps_needs_its_argument(tmp_path):
    r = subprocess.run([RAFT, "-e", "30", "--repeat-overlaps"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1 and r.stdout.decode() == USAGE
