"""GPU: `raft -e auto` -- the estimated coverage read from the data (a survey pass, its coverage histogram on the device,
raft_hip_estimate_coverage) -- gives exactly the run of `raft -e N` with the N it found, and N is what the specification gives on the
oracle's coverage."""
import os
import subprocess

import numpy as np
import pytest
from raft_testlib import ROOT, oracle_run, write_fasta, write_paf
from test_cov_estimate import restate

from raft_amd.params import RaftParams

pytestmark = pytest.mark.gpu
RAFT = os.path.join(ROOT, "raft_amd", "bin", "raft")
FILES = ("reads.fasta", "coverage.txt", "long_repeats.txt", "long_repeats.bed")


def run(cwd, args, env=None):
    r = subprocess.run([RAFT] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300,
                       env=dict(os.environ, **env) if env else None)
    return r.returncode, r.stdout.decode()


def comparable(out):
    """stdout without the lines that differ by construction: how est_cov was given, the estimate, the timer, the command line."""
    drop = ("INFO, printParams(), est_cov = ", "INFO, estimate_coverage(), est_cov = ", "INFO, main(), program completed after", "INFO, main(), CMD:")
    return [l for l in out.split("\n") if not l.startswith(drop)]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    from raft_amd.synth import make_overlaps
    d = tmp_path_factory.mktemp("cli_auto")
    o = make_overlaps(4000, coverage=30, seed=3)
    cols = [c.numpy() for c in (o.read_len,) + o.columns()]
    names = [f"r{i}" for i in range(o.n_reads)]
    write_fasta(d / "reads.fa", names, cols[0])
    write_paf(d / "overlaps.paf", names, *cols)
    cov = oracle_run(RaftParams(est_cov=30), *cols)["cov"]
    n = restate(np.bincount(np.minimum(cov, 4095), minlength=4096))["est_cov"]
    assert n > 0
    rc, out = run(d, ["-e", str(n), "-o", "b", "reads.fa", "overlaps.paf"])
    assert rc == 0, out
    return d, n, out


@pytest.mark.parametrize("env", [None, {"RAFT_DEVICES": "0,0"}], ids=["one", "two-contexts"])
def test_auto_equals_the_run_with_its_estimate(inputs, env):
    d, n, out_b = inputs
    rc, out = run(d, ["-e", "auto", "-o", "a", "reads.fa", "overlaps.paf"], env)
    assert rc == 0, out
    lines = out.split("\n")
    assert "INFO, printParams(), est_cov = auto" in lines
    assert f"INFO, estimate_coverage(), est_cov = {n}" in lines
    assert f"INFO, printParams(), est_cov = {n}" in out_b.split("\n")
    assert lines.index(f"INFO, estimate_coverage(), est_cov = {n}") < [i for i, l in enumerate(lines) if l.startswith("INFO, Symmetric overlaps")][0]
    assert comparable(out) == comparable(out_b)
    for f in FILES:
        a, b = open(d / ("a." + f), "rb").read(), open(d / ("b." + f), "rb").read()
        assert a == b, f
        assert len(a) > 0 or f == "long_repeats.bed", f      # (the .bed is written for simulated reads only, repeat.hpp:180-203: empty here)
        os.remove(d / ("a." + f))


def test_no_covered_window_is_the_unset_error(tmp_path):
    (tmp_path / "a.fa").write_text(">x\n" + "ACGT" * 100 + "\n")
    (tmp_path / "b.paf").write_text("x\t400\t0\t0\t+\tx\t400\t0\t0\t1\t1\t1\n")     # qs = qe = 0: the record covers no window
    rc, out = run(tmp_path, ["-e", "auto", "a.fa", "b.paf"])
    assert rc == 1, out
    assert "INFO, printParams(), est_cov = auto\n" in out
    assert "ERROR, main(), estimated coverage must be set properly\nUsage: raft [options] <input-reads.fa> <in.paf>\n" in out
    assert "estimate_coverage()" not in out and "Symmetric overlaps" not in out


def test_a_data_error_in_the_survey_reads_as_the_jobs(tmp_path):
    (tmp_path / "a.fa").write_text(">x\nACGT\n")
    (tmp_path / "b.paf").write_text("x\t4\t0\t400\t+\tx\t4\t0\t4\t1\t1\t1\n")        # reaches past the last window
    rc, out_n = run(tmp_path, ["-e", "30", "a.fa", "b.paf"])
    rc_a, out_a = run(tmp_path, ["-e", "auto", "a.fa", "b.paf"])
    assert rc == 1 and rc_a == 1
    err = [l for l in out_n.split("\n") if l.startswith("ERROR")]
    assert len(err) == 1 and err[0].startswith("ERROR, raft_hip, PAF coordinate")
    assert [l for l in out_a.split("\n") if l.startswith("ERROR")] == err


@pytest.mark.parametrize("value", ["0", "autox", "Auto", "-3"])
def test_other_values_keep_todays_error(tmp_path, value):
    rc, out = run(tmp_path, ["-e", value, "a.fa", "b.paf"])
    assert rc == 1 and out.startswith("ERROR, main(), estimated coverage must be set properly\nUsage: raft [options] <input-reads.fa> <in.paf>\n")
    rc, out = run(tmp_path, ["a.fa", "b.paf"])
    assert rc == 1 and out.startswith("ERROR, main(), estimated coverage must be set properly\nUsage:")
