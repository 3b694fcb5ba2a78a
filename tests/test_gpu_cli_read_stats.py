"""GPU: `raft --read-stats` -- PREFIX.read_stats.tsv, the per-read table (raft_hip_read_stats on a survey pass, raft_hip_census_host on the
tokenised columns, the job's own repeats and fragments).  On the micro fixtures the reference's four files and its stdout stay what they
are, and every column of the table equals what the fixture's own files and its PAF text give."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
from raft_testlib import GOLDEN, ROOT, parse_coverage_txt, parse_fasta_headers, parse_long_repeats, write_fasta, write_paf

pytestmark = pytest.mark.gpu
RAFT = os.path.join(ROOT, "raft_amd", "bin", "raft")
MAN = json.load(open(os.path.join(GOLDEN, "manifest.json")))
HEADER = ["read", "name", "length", "windows", "intervals", "contained", "cov_sum", "cov_max", "high_windows", "repeats", "fragments"]
FILES = ("reads.fasta", "coverage.txt", "long_repeats.txt", "long_repeats.bed")


def run(cwd, args):
    r = subprocess.run([RAFT] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    return r.returncode, r.stdout.decode()


def strip_timing(out):
    return "\n".join(l for l in out.split("\n")
                     if not l.startswith("INFO, main(), program completed after") and not l.startswith("INFO, main(), CMD:"))


def read_fasta(path):
    """names (to the first white space) and lengths of a FASTA file."""
    names, lens = [], []
    for line in open(path).read().split("\n"):
        if line.startswith(">"):
            names.append(line[1:].split()[0])
            lens.append(0)
        elif names:
            lens[-1] += len(line.strip())
    return names, np.array(lens, np.int64)


def read_paf(path, names):
    """The six integer columns of the lines with ten fields or more."""
    ids = {n: i for i, n in enumerate(names)}
    rows = []
    for line in open(path).read().split("\n"):
        f = line.split("\t")
        if len(f) >= 10:
            rows.append((ids[f[0]], int(f[2]), int(f[3]), ids[f[5]], int(f[7]), int(f[8])))
    return [np.array([r[k] for r in rows], np.int64) for k in range(6)]


def read_tsv(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and lines[0].split("\t") == HEADER
    rows = [l.split("\t") for l in lines[1:-1]]
    assert all(len(r) == len(HEADER) for r in rows)
    return {h: [r[k] if h == "name" else int(r[k]) for r in rows] for k, h in enumerate(HEADER)}


def fragments_per_read(fasta_text, names):
    if all("," in n for n in names):                       # simulated reads: the header names orientation and contig, not the read
        key = {(n.split(",")[1], n.split(",")[-1]): i for i, n in enumerate(names)}
        out = [0] * len(names)
        for line in fasta_text.split("\n"):
            if line.startswith(">"):
                f = line[1:].split(",")
                out[key[(f[1], f[-1])]] += 1
        return out
    index = {n: i for i, n in enumerate(names)}
    out = [0] * len(names)
    for _, name, _, _ in parse_fasta_headers(fasta_text):
        out[index[name]] += 1
    return out


@pytest.mark.parametrize("name", ["g1", "g2", "g3", "g4"])
def test_micro_fixtures(tmp_path, name):
    d = os.path.join(GOLDEN, "micro", name)
    meta = MAN["micro"][name]
    shutil.copy(os.path.join(d, "reads.fa"), tmp_path)
    shutil.copy(os.path.join(d, "overlaps.paf"), tmp_path)
    rc, out = run(tmp_path, meta["args"] + ["--read-stats", "reads.fa", "overlaps.paf"])
    assert rc == 0, out
    # the reference's files and lines are what they are without the option
    produced = sorted(f for f in os.listdir(tmp_path) if f not in ("reads.fa", "overlaps.paf"))
    assert produced == sorted(meta["outputs"] + ["raft.read_stats.tsv"])
    for f in meta["outputs"]:
        assert open(tmp_path / f, "rb").read() == open(os.path.join(d, "expect." + f), "rb").read(), (name, f)
    lines = strip_timing(out).split("\n")
    added = [l for l in lines if l.startswith("INFO, read_stats(), ")]
    assert len(added) == 1 and lines[-2] == added[0] and lines[-1] == ""
    assert "\n".join(l for l in lines if l is not added[0]) == open(os.path.join(d, "expect.stdout")).read()

    names, length = read_fasta(tmp_path / "reads.fa")
    qid, qs, qe, tid, ts, te = read_paf(tmp_path / "overlaps.paf", names)
    args = dict(zip(meta["args"][::2], meta["args"][1::2]))
    reso = int(args["-r"])
    symmetric = int([l for l in lines if l.startswith("INFO, Symmetric overlaps")][0].split()[3])
    high_cov = int([l for l in lines if l.startswith("high_cov ")][0].split()[1])
    assert high_cov >= 1
    t = read_tsv(tmp_path / "raft.read_stats.tsv")
    n = len(names)
    assert t["read"] == list(range(n)) and t["name"] == names and t["length"] == list(length)
    assert t["windows"] == list((length + reso - 1) // reso)
    cov = parse_coverage_txt(open(os.path.join(d, "expect.raft.coverage.txt")).read())
    assert t["cov_sum"] == [int(c.sum()) for c in cov]
    assert t["cov_max"] == [int(c.max(initial=0)) for c in cov]
    assert t["high_windows"] == [int((c >= high_cov).sum()) for c in cov]
    assert t["repeats"] == [len(r) for r in parse_long_repeats(open(os.path.join(d, "expect.raft.long_repeats.txt")).read())]
    assert t["fragments"] == fragments_per_read(open(os.path.join(d, "expect.raft.reads.fasta")).read(), names)
    intervals = np.bincount(qid, minlength=n)
    flags = np.zeros(n, np.int64)
    q_side = np.zeros(n, bool)
    np.logical_or.at(q_side, qid, (qs == 0) & (qe == length[qid]) & (length[tid] > length[qid]))
    flags[q_side] |= 1
    if not symmetric:
        intervals = intervals + np.bincount(tid[tid != qid], minlength=n)
        t_side = np.zeros(n, bool)
        np.logical_or.at(t_side, tid, (ts == 0) & (te == length[tid]) & (length[qid] > length[tid]))
        flags[t_side] |= 2
    assert t["intervals"] == list(intervals) and t["contained"] == list(flags)
    assert added[0] == f"INFO, read_stats(), contained reads = {int((flags != 0).sum())} of {n}"


def test_no_table_without_the_option(tmp_path):
    d = os.path.join(GOLDEN, "micro", "g1")
    meta = MAN["micro"]["g1"]
    shutil.copy(os.path.join(d, "reads.fa"), tmp_path)
    shutil.copy(os.path.join(d, "overlaps.paf"), tmp_path)
    rc, out = run(tmp_path, meta["args"] + ["reads.fa", "overlaps.paf"])
    assert rc == 0, out
    assert sorted(f for f in os.listdir(tmp_path) if f not in ("reads.fa", "overlaps.paf")) == meta["outputs"]
    assert "read_stats" not in out and strip_timing(out) == open(os.path.join(d, "expect.stdout")).read()


def test_auto_and_read_stats_equal_the_run_with_the_estimate(tmp_path):
    from raft_amd.synth import make_overlaps
    o = make_overlaps(1500, coverage=30, seed=3)
    cols = [c.numpy() for c in (o.read_len,) + o.columns()]
    names = [f"r{i}" for i in range(o.n_reads)]
    write_fasta(tmp_path / "reads.fa", names, cols[0])
    write_paf(tmp_path / "overlaps.paf", names, *cols)
    rc, out = run(tmp_path, ["-e", "auto", "--read-stats", "-o", "a", "reads.fa", "overlaps.paf"])
    assert rc == 0, out
    est = [l for l in out.split("\n") if l.startswith("INFO, estimate_coverage(), est_cov = ")]
    assert len(est) == 1
    n = int(est[0].split()[-1])
    assert n > 0
    rc, out_b = run(tmp_path, ["-e", str(n), "--read-stats", "-o", "b", "reads.fa", "overlaps.paf"])
    assert rc == 0, out_b
    for f in FILES + ("read_stats.tsv",):
        a, b = open(tmp_path / ("a." + f), "rb").read(), open(tmp_path / ("b." + f), "rb").read()
        assert a == b, f
    t = read_tsv(tmp_path / "a.read_stats.tsv")
    assert t["name"] == names and sum(t["cov_sum"]) > 0 and max(t["high_windows"]) > 0
    assert [l for l in out.split("\n") if l.startswith("INFO, read_stats()")] == [l for l in out_b.split("\n") if l.startswith("INFO, read_stats()")]
