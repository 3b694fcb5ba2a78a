"""GPU: `raft --overlap-ends H --string-graph [--string-graph-fuzz Z]` -- PREFIX.string_graph.gfa, PREFIX.string_graph.tsv and the
option's stdout line against the Python writer of tests/test_string_graph_writer.py over the plain-Python rule of tests/sg_testlib.py
over ``hostio.load_paf(strand=True)``, the contained reads of ``want_all`` left out; beside the filter (the strand follows the kept
records), under RAFT_CLI_PREPARE=1 and on two contexts; beside every other option; without the flag every file and all of stdout those
of the same command; the usage errors; and the two-step recipe on the fragments.  On the 300-read, 30-fold set of
tests/test_gpu_cli_lift.py.  Every run goes under a time limit of its own, and nothing more is started after one that aborted, faulted
or ran into it."""
import os
import subprocess

import numpy as np
import pytest
from sg_testlib import oracle
from test_gpu_cli_all_options import ROWS, option_lines
from test_gpu_cli_filter import keeps
from test_gpu_cli_lift import dataset  # noqa: F401  (the fixture)
from test_gpu_cli_overlap_ends import CMD, FILES, RAFT, files_of, strip_timing
from test_gpu_overlap_ends import want_all
from test_string_graph_writer import gfa_text, tsv_text

from raft_amd import hostio

pytestmark = pytest.mark.gpu
LINE = "INFO, string_graph(), "
OURS = ("string_graph.gfa", "string_graph.tsv")
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


def expected(d, fasta, paf, H=100, F=800, fuzz=1000, keep=None):
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
    status = want_all(rl, cols[:6], cols[6], H, F, bool(sym))[2]
    skip = (status == 1).astype(np.uint8)                                  # overlap_ends' `contained`
    w = oracle(rl, cols[:6], cols[6], H, F, fuzz, bool(sym), skip)
    s = w["summary"]
    line = (f"{LINE}fuzz = {fuzz}, records = {s['records']}, dovetail views = {s['dovetail_views']}, left out = {s['views_left_out']}, "
            f"arcs = {s['arcs']}, duplicates = {s['duplicate_arcs']}, unpaired = {s['unpaired_arcs']}, reducible = {s['reducible_arcs']}, "
            f"edges = {s['edges']}, kept = {s['kept_edges']}, ends with one = {s['ends_kept_one']}, ends that branch = {s['ends_kept_more']}, "
            f"dead ends = {s['ends_dead']}, mutual ends = {s['ends_mutual']}, reads left out = {s['reads_flagged']} of {len(names)}, "
            f"longest row = {s['longest_row']}")
    return gfa_text(names, rl.tolist(), w).encode(), tsv_text(names, rl.tolist(), w).encode(), line, w


def check_run(d, prefix, out, want):
    gfa, tsv, line, _ = want
    lines = out.split("\n")
    assert lines[-1] == "" and lines[-2] == line and sum(l.startswith(LINE) for l in lines) == 1, (lines[-4:], line)
    assert open(d / f"{prefix}.string_graph.gfa", "rb").read() == gfa
    assert open(d / f"{prefix}.string_graph.tsv", "rb").read() == tsv


def test_the_files_and_the_line_equal_the_oracle(dataset):  # noqa: F811
    d = dataset[0]
    _, out = run(d, ["-e", EST, "--overlap-ends", "100", "--string-graph", "-o", "ga", "reads.fa", "overlaps.paf"])
    want = expected(d, "reads.fa", "overlaps.paf")
    s = want[3]["summary"]
    assert s["reducible_arcs"] >= 1 and s["kept_edges"] >= 1 and s["reads_flagged"] >= 1 and s["views_left_out"] >= 1, s
    check_run(d, "ga", out, want)
    assert files_of(d, "ga") == sorted(FILES + ENDS + OURS)
    # without the flag: every file and all of stdout, byte for byte
    _, plain = run(d, ["-e", EST, "--overlap-ends", "100", "-o", "gb", "reads.fa", "overlaps.paf"])
    assert LINE not in plain and strip_timing("\n".join(out.split("\n")[:-2] + [""])) == strip_timing(plain)
    assert files_of(d, "gb") == sorted(FILES + ENDS)
    for f in FILES + ENDS:
        assert open(d / f"ga.{f}", "rb").read() == open(d / f"gb.{f}", "rb").read(), f


@pytest.mark.parametrize("fuzz", [0, 37, 2147483647])
def test_the_fuzz(dataset, fuzz):  # noqa: F811
    d = dataset[0]
    _, out = run(d, ["-e", EST, "--overlap-ends", "100", "--string-graph", "--string-graph-fuzz", str(fuzz), "-o", f"gz{fuzz}", "reads.fa", "overlaps.paf"])
    check_run(d, f"gz{fuzz}", out, expected(d, "reads.fa", "overlaps.paf", fuzz=fuzz))


@pytest.mark.parametrize("condition", ["filter", "cli_prepare", "two_contexts"])
def test_beside_the_filter_prepared_and_on_two_contexts(dataset, condition):  # noqa: F811
    d = dataset[0]
    extra = ["--min-identity", "99", "--min-overlap", "500"] if condition == "filter" else []
    env = {"cli_prepare": {"RAFT_CLI_PREPARE": "1"}, "two_contexts": {"RAFT_DEVICES": "0,0"}}.get(condition, {})
    _, out = run(d, ["-e", EST] + extra + ["--overlap-ends", "100", "--string-graph", "-o", f"g_{condition}", "reads.fa", "overlaps.paf"], **env)
    keep = None
    if condition == "filter":
        keep = np.array([keeps(l, 990, 500) for l in (d / "overlaps.paf").read_text().splitlines()])
        assert 0 < keep.sum() < keep.size
    want = expected(d, "reads.fa", "overlaps.paf", keep=keep)
    check_run(d, f"g_{condition}", out, want)
    if keep is not None:
        assert want[3]["summary"]["records"] == int(keep.sum())


def test_beside_every_other_option(dataset):  # noqa: F811
    d = dataset[0]
    every = [a for _, args, _ in ROWS for a in args] + ["--components"]
    _, out = run(d, ["-e", EST] + every + ["--string-graph", "-o", "g_all", "reads.fa", "overlaps.paf"])
    got = option_lines(out.split("\n"))
    names = [n for n, _, _ in ROWS]
    at = names.index("unitigs") + 1
    assert [n for n, _ in got] == names[:at] + ["components", "string_graph"] + names[at:], got      # behind components', before fragment_paf's
    assert names[at:] == ["fragment_paf"]
    _, alone = run(d, ["-e", EST, "--overlap-ends", "100", "--string-graph", "-o", "g_one", "reads.fa", "overlaps.paf"])
    assert dict(got)["string_graph"] == alone.split("\n")[-2]
    theirs = tuple(f for _, _, fs in ROWS for f in fs) + ("components.tsv", "components.summary.tsv")
    assert files_of(d, "g_all") == sorted(FILES + theirs + OURS)
    for f in OURS:
        assert open(d / f"g_all.{f}", "rb").read() == open(d / f"g_one.{f}", "rb").read(), f
    # ... and the other options' files and lines are those of the run without the flag
    _, without = run(d, ["-e", EST] + every + ["-o", "g_none", "reads.fa", "overlaps.paf"])
    assert [l for l in out.split("\n") if not l.startswith(LINE) and not l.startswith(CMD) and "program completed after" not in l] == \
           [l for l in without.split("\n") if not l.startswith(CMD) and "program completed after" not in l]
    assert files_of(d, "g_none") == sorted(FILES + theirs)
    for f in files_of(d, "g_none"):
        assert open(d / f"g_all.{f}", "rb").read() == open(d / f"g_none.{f}", "rb").read(), f


@pytest.mark.parametrize("args", [["--string-graph"], ["--overlap-ends", "100", "--string-graph-fuzz", "5"]], ids=["without --overlap-ends", "the fuzz without the option"])
def test_the_usage_errors(dataset, args):  # noqa: F811
    d = dataset[0]
    rc, out = run(d, ["-e", EST] + args + ["-o", "g_bad", "reads.fa", "overlaps.paf"], ok=False)
    assert rc == 1 and "Usage: raft [options] <input-reads.fa> <in.paf>" in out and "ERROR" not in out
    assert files_of(d, "g_bad") == []


def test_the_two_step_recipe_on_the_fragments(dataset):  # noqa: F811
    d = dataset[0]
    run(d, ["-e", EST, "--fragment-paf", "-o", "gf", "reads.fa", "overlaps.paf"])
    _, out = run(d, ["-e", "20", "--overlap-ends", "100", "--string-graph", "-o", "gf2", "gf.reads.fasta", "gf.fragments.paf"])
    want = expected(d, "gf.reads.fasta", "gf.fragments.paf")
    check_run(d, "gf2", out, want)
    s = want[3]["summary"]
    assert s["arcs"] > 0 and s["kept_edges"] >= 1 and len(want[3]["flags"]) > 300
