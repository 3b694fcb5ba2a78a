"""GPU: `raft --low-cov C` -- PREFIX.low_coverage.bed, the runs of windows with coverage <= C per read (raft_hip_low_coverage on the
survey pass).  On the micro fixtures the reference's four files and its stdout stay what they are and the BED equals the definition
applied to the fixture's own coverage.txt; with -e auto and --read-stats it is the same pass; without the option nothing is new."""
import json
import os
import shutil

import numpy as np
import pytest
from raft_testlib import GOLDEN, parse_coverage_txt, write_fasta, write_paf
from test_gpu_cli_read_stats import FILES, read_fasta, run, strip_timing
from test_low_cov_cases import INTERIOR, UNCOVERED, want_low
from test_low_cov_writer import restate_bed

pytestmark = pytest.mark.gpu
MAN = json.load(open(os.path.join(GOLDEN, "manifest.json")))
LINE = "INFO, low_coverage(), "


def expected(cov_per_read, length, reso, low_cov):
    want = {"cov": np.concatenate([np.asarray(c, np.int64) for c in cov_per_read] + [np.empty(0, np.int64)]),
            "cov_offset": np.concatenate([[0], np.cumsum([len(c) for c in cov_per_read])]).astype(np.int64)}
    return want_low(want, length, reso, low_cov, 800)


def the_line(w, low_cov, n_reads):
    return (f"{LINE}low_cov = {low_cov}, runs = {w['n_runs']}, reads with an interior run = {w['reads_interior']}, "
            f"uncovered reads = {w['reads_uncovered']} of {n_reads}")


@pytest.mark.parametrize("low_cov", [0, 1])
@pytest.mark.parametrize("name", ["g1", "g2", "g3", "g4"])
def test_micro_fixtures(tmp_path, name, low_cov):
    d = os.path.join(GOLDEN, "micro", name)
    meta = MAN["micro"][name]
    shutil.copy(os.path.join(d, "reads.fa"), tmp_path)
    shutil.copy(os.path.join(d, "overlaps.paf"), tmp_path)
    rc, out = run(tmp_path, meta["args"] + ["--low-cov", str(low_cov), "reads.fa", "overlaps.paf"])
    assert rc == 0, out
    produced = sorted(f for f in os.listdir(tmp_path) if f not in ("reads.fa", "overlaps.paf"))
    assert produced == sorted(meta["outputs"] + ["raft.low_coverage.bed"])
    for f in meta["outputs"]:
        assert open(tmp_path / f, "rb").read() == open(os.path.join(d, "expect." + f), "rb").read(), (name, f)
    lines = strip_timing(out).split("\n")
    added = [l for l in lines if l.startswith(LINE)]
    assert len(added) == 1 and lines[-2] == added[0] and lines[-1] == ""
    assert "\n".join(l for l in lines if l is not added[0]) == open(os.path.join(d, "expect.stdout")).read()

    names, length = read_fasta(tmp_path / "reads.fa")
    args = dict(zip(meta["args"][::2], meta["args"][1::2]))
    reso = int(args["-r"])
    cov = parse_coverage_txt(open(os.path.join(d, "expect.raft.coverage.txt")).read())
    w = expected(cov, length, reso, low_cov)
    assert open(tmp_path / "raft.low_coverage.bed").read() == restate_bed(names, w["low_offset"], w["low_s"], w["low_e"], length)
    assert added[0] == the_line(w, low_cov, len(names))
    assert w["reads_interior"] == int(((w["low_flags"] & INTERIOR) != 0).sum()) and w["reads_uncovered"] == int(((w["low_flags"] & UNCOVERED) != 0).sum())


def _synthetic(tmp_path):
    from raft_amd.synth import make_overlaps
    o = make_overlaps(1500, coverage=30, seed=3)
    cols = [c.numpy() for c in (o.read_len,) + o.columns()]
    names = [f"r{i}" for i in range(o.n_reads)]
    write_fasta(tmp_path / "reads.fa", names, cols[0])
    write_paf(tmp_path / "overlaps.paf", names, *cols)
    return names, cols


def test_auto_read_stats_and_low_cov_equal_the_run_with_the_estimate(tmp_path):
    names, cols = _synthetic(tmp_path)
    rc, out = run(tmp_path, ["-e", "auto", "--low-cov", "0", "--read-stats", "-o", "a", "reads.fa", "overlaps.paf"])
    assert rc == 0, out
    est = [l for l in out.split("\n") if l.startswith("INFO, estimate_coverage(), est_cov = ")]
    assert len(est) == 1
    n = int(est[0].split()[-1])
    assert n > 0
    rc, out_b = run(tmp_path, ["-e", str(n), "--low-cov", "0", "--read-stats", "-o", "b", "reads.fa", "overlaps.paf"])
    assert rc == 0, out_b
    for f in FILES + ("read_stats.tsv", "low_coverage.bed"):
        assert open(tmp_path / ("a." + f), "rb").read() == open(tmp_path / ("b." + f), "rb").read(), f
    tail_a, tail_b = strip_timing(out).split("\n")[-3:], strip_timing(out_b).split("\n")[-3:]
    assert tail_a == tail_b and tail_a[0].startswith("INFO, read_stats(), ") and tail_a[1].startswith(LINE) and tail_a[2] == ""
    # ... and the BED is the definition applied to the job's own coverage.txt
    cov = parse_coverage_txt(open(tmp_path / "a.coverage.txt").read())
    w = expected(cov, cols[0], 50, 0)
    assert w["n_runs"] > 0
    assert open(tmp_path / "a.low_coverage.bed").read() == restate_bed(names, w["low_offset"], w["low_s"], w["low_e"], cols[0])
    assert tail_a[1] == the_line(w, 0, len(names))


def test_nothing_new_without_the_option(tmp_path):
    _synthetic(tmp_path)
    rc, out = run(tmp_path, ["-e", "30", "reads.fa", "overlaps.paf"])
    assert rc == 0, out
    assert sorted(f for f in os.listdir(tmp_path) if f not in ("reads.fa", "overlaps.paf")) == sorted("raft." + f for f in FILES)
    assert "low_coverage" not in out
    d = os.path.join(GOLDEN, "micro", "g1")
    meta = MAN["micro"]["g1"]
    sub = tmp_path / "g1"
    sub.mkdir()
    shutil.copy(os.path.join(d, "reads.fa"), sub)
    shutil.copy(os.path.join(d, "overlaps.paf"), sub)
    rc, out = run(sub, meta["args"] + ["reads.fa", "overlaps.paf"])
    assert rc == 0, out
    assert sorted(f for f in os.listdir(sub) if f not in ("reads.fa", "overlaps.paf")) == meta["outputs"]
    assert strip_timing(out) == open(os.path.join(d, "expect.stdout")).read()
