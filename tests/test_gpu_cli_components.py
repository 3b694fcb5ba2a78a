"""GPU: `raft --overlap-ends H --components` -- PREFIX.components.tsv, PREFIX.components.summary.tsv and the option's stdout line
against the sequential union-find of tests/cc_testlib.py over ``hostio.load_paf(strand=True)``; beside the filter, under
RAFT_CLI_PREPARE=1 and on two contexts; beside every other option; without the flag every file and all of stdout those of the same
command; the usage error; and the two-step recipe on the fragments.  On the 300-read, 30-fold set of tests/test_gpu_cli_lift.py.  Every
run goes under a time limit of its own, and nothing more is started after one that aborted, faulted or ran into it."""
import os
import subprocess

import numpy as np
import pytest
from cc_testlib import KINDS_PROPER, oracle
from test_gpu_cli_all_options import ROWS, option_lines
from test_gpu_cli_filter import keeps
from test_gpu_cli_lift import dataset  # noqa: F401  (the fixture)
from test_gpu_cli_overlap_ends import CMD, FILES, RAFT, files_of, strip_timing

from raft_amd import hostio

pytestmark = pytest.mark.gpu
LINE = "INFO, components(), "
OURS = ("components.tsv", "components.summary.tsv")
ENDS = ("overlap_ends.tsv",)
EST = "30"
FATAL = (134, 139, 124, 137)          # abort, segmentation fault, the time limit (and its kill)
stopped = []                          # the run after which nothing more is started


def run(d, args, ok=True, **env):
    if stopped:
        pytest.fail(f"not started: an earlier run ended with {stopped[0]}")
    r = subprocess.run(["timeout", "-k", "10", "60", RAFT] + args, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **env))
    if r.returncode in FATAL:
        stopped.append(f"exit code {r.returncode}: raft {' '.join(args)} under {env}")
        pytest.fail(stopped[0] + "\n" + r.stdout.decode()[-2000:] + r.stderr.decode()[-2000:])
    if ok:
        assert r.returncode == 0, (args, env, r.stdout.decode()[-2000:], r.stderr.decode()[-2000:])
    return r.returncode, r.stdout.decode()


def expected(d, fasta, paf, H=100, F=800, keep=None):
    """-> the bytes of the two files, the stdout line and the oracle's result, from the oracle over the tokenised file"""
    reads = hostio.Reads(str(d / fasta))
    try:
        names, rl = [reads.name(i) for i in range(reads.n)], np.array(reads.lengths, np.int32)
        cols, sym = hostio.load_paf(str(d / paf), reads, with_flag=True, strand=True)
        if keep is not None:
            cols = [c[keep] for c in cols]
            src = d / f"kept_{paf}"
            src.write_text("".join(l + "\n" for l, k in zip((d / paf).read_text().splitlines(), keep) if k))
            sym = hostio.load_paf(str(src), reads, with_flag=True)[1]       # (the flag of the kept stream)
    finally:
        reads.close()
    w = oracle(rl, cols[:6], cols[6], H, F, KINDS_PROPER, bool(sym))
    s = w["summary"]
    per_read = "".join(f"{names[r]}\t{int(rl[r])}\t{int(w['component'][r])}\t{int(w['degree'][r])}\n" for r in range(len(names)))
    per_comp = "".join(f"{k}\t{int(w['comp_reads'][k])}\t{int(w['comp_bases'][k])}\t{int(w['comp_sides'][k])}\t{names[int(w['comp_first'][k])]}\n"
                       for k in range(s["components"]))
    line = (f"{LINE}kinds = {KINDS_PROPER}, records = {s['n_records']}, edges = {s['edge_records']}, components = {s['components']}, "
            f"singletons = {s['singletons']}, largest = {s['largest_reads']} reads, largest bases = {s['largest_bases']} of {s['total_bases']}, "
            f"reads in the largest = {s['reads_in_largest_permille']} per mille of {s['n_reads']}")
    return per_read.encode(), per_comp.encode(), line, w


def check_run(d, prefix, out, want):
    per_read, per_comp, line, _ = want
    lines = out.split("\n")
    assert lines[-1] == "" and lines[-2] == line and sum(l.startswith(LINE) for l in lines) == 1, (lines[-4:], line)
    assert open(d / f"{prefix}.components.tsv", "rb").read() == per_read
    assert open(d / f"{prefix}.components.summary.tsv", "rb").read() == per_comp


def test_the_files_and_the_line_equal_the_oracle(dataset):  # noqa: F811
    d = dataset[0]
    _, out = run(d, ["-e", EST, "--overlap-ends", "100", "--components", "-o", "ca", "reads.fa", "overlaps.paf"])
    want = expected(d, "reads.fa", "overlaps.paf")
    s = want[3]["summary"]
    assert 0 < s["edge_records"] < s["n_records"] and 1 <= s["components"] < 300 and s["largest_reads"] > 1
    check_run(d, "ca", out, want)
    assert files_of(d, "ca") == sorted(FILES + ENDS + OURS)
    # without the flag: every file and all of stdout, byte for byte
    _, plain = run(d, ["-e", EST, "--overlap-ends", "100", "-o", "cb", "reads.fa", "overlaps.paf"])
    assert LINE not in plain and strip_timing("\n".join(out.split("\n")[:-2] + [""])) == strip_timing(plain)
    assert files_of(d, "cb") == sorted(FILES + ENDS)
    for f in FILES + ENDS:
        assert open(d / f"ca.{f}", "rb").read() == open(d / f"cb.{f}", "rb").read(), f


@pytest.mark.parametrize("condition", ["filter", "cli_prepare", "two_contexts"])
def test_beside_the_filter_prepared_and_on_two_contexts(dataset, condition):  # noqa: F811
    d = dataset[0]
    extra = ["--min-identity", "99", "--min-overlap", "500"] if condition == "filter" else []
    env = {"cli_prepare": {"RAFT_CLI_PREPARE": "1"}, "two_contexts": {"RAFT_DEVICES": "0,0"}}.get(condition, {})
    _, out = run(d, ["-e", EST] + extra + ["--overlap-ends", "100", "--components", "-o", f"c_{condition}", "reads.fa", "overlaps.paf"], **env)
    keep = None
    if condition == "filter":
        keep = np.array([keeps(l, 990, 500) for l in (d / "overlaps.paf").read_text().splitlines()])
        assert 0 < keep.sum() < keep.size
    want = expected(d, "reads.fa", "overlaps.paf", keep=keep)
    check_run(d, f"c_{condition}", out, want)
    if keep is not None:
        assert want[3]["summary"]["n_records"] == int(keep.sum())


def test_beside_every_other_option(dataset):  # noqa: F811
    d = dataset[0]
    every = [a for _, args, _ in ROWS for a in args]
    _, out = run(d, ["-e", EST] + every + ["--components", "-o", "c_all", "reads.fa", "overlaps.paf"])
    got = option_lines(out.split("\n"))
    names = [n for n, _, _ in ROWS]
    at = names.index("unitigs") + 1
    assert [n for n, _ in got] == names[:at] + ["components"] + names[at:], got      # behind unitigs', before fragment_paf's
    _, alone = run(d, ["-e", EST, "--overlap-ends", "100", "--components", "-o", "c_one", "reads.fa", "overlaps.paf"])
    assert dict(got)["components"] == alone.split("\n")[-2]
    assert files_of(d, "c_all") == sorted(FILES + tuple(f for _, _, fs in ROWS for f in fs) + OURS)
    for f in OURS:
        assert open(d / f"c_all.{f}", "rb").read() == open(d / f"c_one.{f}", "rb").read(), f
    # ... and the other options' files and lines are those of the run without the flag
    _, without = run(d, ["-e", EST] + every + ["-o", "c_none", "reads.fa", "overlaps.paf"])
    assert [l for l in out.split("\n") if not l.startswith(LINE) and not l.startswith(CMD) and "program completed after" not in l] == \
           [l for l in without.split("\n") if not l.startswith(CMD) and "program completed after" not in l]
    for f in files_of(d, "c_none"):
        assert open(d / f"c_all.{f}", "rb").read() == open(d / f"c_none.{f}", "rb").read(), f


def test_without_overlap_ends_it_is_a_usage_error(dataset):  # noqa: F811
    d = dataset[0]
    rc, out = run(d, ["-e", EST, "--components", "-o", "c_bad", "reads.fa", "overlaps.paf"], ok=False)
    assert rc == 1 and "Usage: raft [options] <input-reads.fa> <in.paf>" in out and "ERROR" not in out
    assert files_of(d, "c_bad") == []


def test_the_two_step_recipe_on_the_fragments(dataset):  # noqa: F811
    d = dataset[0]
    run(d, ["-e", EST, "--fragment-paf", "-o", "cf", "reads.fa", "overlaps.paf"])
    _, out = run(d, ["-e", "20", "--overlap-ends", "100", "--components", "-o", "cf2", "cf.reads.fasta", "cf.fragments.paf"])
    want = expected(d, "cf.reads.fasta", "cf.fragments.paf")
    check_run(d, "cf2", out, want)
    s = want[3]["summary"]
    assert s["n_reads"] > 300 and s["edge_records"] > 0 and s["components"] >= 1
