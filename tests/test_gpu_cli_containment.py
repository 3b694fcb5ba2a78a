"""GPU: `raft --overlap-ends H --containment [--best-overlaps --unitigs]` -- PREFIX.containment.tsv, PREFIX.unitigs.depth.tsv and the two
stdout lines against the Python format of tests/test_containment_writer.py over the sequential walk of tests/ctn_testlib.py over
``hostio.load_paf(strand=True)``; the placed columns from that forest laid by ``place_oracle`` onto the layout the run's own unitig files
state; beside the filter, under RAFT_CLI_PREPARE=1 and on two contexts; beside every other option; without the flag every file and all
of stdout those of the same command; the usage errors; and the two-step recipe on the fragments.  On the 300-read, 30-fold set of
tests/test_gpu_cli_lift.py.  Every run goes under a time limit of its own, and nothing more is started after one that aborted, faulted
or ran into it."""
import os
import subprocess

import numpy as np
import pytest
from ctn_testlib import oracle, place_oracle
from test_containment_writer import containment_text, depth_text
from test_gpu_cli_all_options import ROWS, option_lines
from test_gpu_cli_filter import keeps
from test_gpu_cli_lift import dataset  # noqa: F401  (the fixture)
from test_gpu_cli_overlap_ends import CMD, FILES, RAFT, files_of, strip_timing

from raft_amd import hostio

pytestmark = pytest.mark.gpu
LINE, PLACE_LINE = "INFO, containment(), ", "INFO, place_contained(), "
OURS, DEPTH = ("containment.tsv",), ("unitigs.depth.tsv",)
ENDS = ("overlap_ends.tsv",)
LAYOUT = ("best_overlaps.tsv", "unitigs.tsv", "unitigs.layout.tsv")
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


def layout_of(d, prefix, names):
    """The layout as the run's unitig files state it: per read unitig, offset, orient; per unitig reads and length"""
    at = {n: i for i, n in enumerate(names)}
    unitig, offset, orient = np.full(len(names), -1, np.int32), np.zeros(len(names), np.int64), np.zeros(len(names), np.uint8)
    for line in (d / f"{prefix}.unitigs.layout.tsv").read_text().splitlines():
        u, _, name, _, o, off = line.split("\t")
        unitig[at[name]], offset[at[name]], orient[at[name]] = int(u), int(off), o == "-"
    rows = [line.split("\t") for line in (d / f"{prefix}.unitigs.tsv").read_text().splitlines()]
    return unitig, offset, orient, np.array([int(r[1]) for r in rows], np.int32), np.array([int(r[2]) for r in rows], np.int64)


def expected(d, fasta, paf, H=100, F=800, keep=None, layout=None):
    """-> the bytes of the file(s), the stdout line(s) and the oracle's results, from the oracle over the tokenised file"""
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
    w = oracle(rl, cols[:6], cols[6], H, F, bool(sym))
    s = w["summary"]
    line = (f"{LINE}records = {s['records']}, containment views = {s['containment_views']}, not longer = {s['views_not_longer']}, "
            f"reads with a parent = {s['reads_with_parent']}, contained without a parent = {s['orphans']}, roots = {s['roots']}, "
            f"roots with a tree = {s['roots_with_tree']}, deepest = {s['greatest_depth']}, largest tree = {s['largest_tree_reads']} reads, "
            f"largest tree bases = {s['largest_tree_bases']}")
    if layout is None:
        return dict(tsv=containment_text(names, rl.tolist(), w).encode(), line=line, forest=w, names=names)
    unitig, offset, orient, utg_reads, utg_length = layout_of(d, layout, names)
    p = place_oracle(rl, w, unitig, offset, orient, utg_length)
    ps = p["summary"]
    place_line = (f"{PLACE_LINE}unitigs = {ps['n_unitigs']}, placed = {ps['placed']}, unplaced = {ps['unplaced']} of {ps['n_reads']}, "
                  f"unitigs that gained reads = {ps['unitigs_gained']}, greatest depth = {ps['greatest_depth_permille']} per mille")
    return dict(tsv=containment_text(names, rl.tolist(), w, p).encode(), depth=depth_text(utg_reads, utg_length, p).encode(), line=line,
                place_line=place_line, forest=w, placed=p, names=names)


def check_run(d, prefix, out, want):
    lines = out.split("\n")
    tail = [want["line"]] + ([want["place_line"]] if "place_line" in want else [])
    assert lines[-1] == "" and lines[-1 - len(tail):-1] == tail, (lines[-4:], tail)
    assert sum(l.startswith(LINE) for l in lines) == 1 and sum(l.startswith(PLACE_LINE) for l in lines) == len(tail) - 1
    assert open(d / f"{prefix}.containment.tsv", "rb").read() == want["tsv"]
    if "depth" in want:
        assert open(d / f"{prefix}.unitigs.depth.tsv", "rb").read() == want["depth"]


def test_the_option_alone(dataset):  # noqa: F811
    d = dataset[0]
    _, out = run(d, ["-e", EST, "--overlap-ends", "100", "--containment", "-o", "ca", "reads.fa", "overlaps.paf"])
    want = expected(d, "reads.fa", "overlaps.paf")
    s = want["forest"]["summary"]
    assert s["reads_with_parent"] >= 1 and s["roots_with_tree"] >= 1 and s["containment_views"] > s["reads_with_parent"], s
    check_run(d, "ca", out, want)
    assert files_of(d, "ca") == sorted(FILES + ENDS + OURS)
    assert all(l.endswith("\t*\t0\t*") for l in want["tsv"].decode().splitlines())
    # without the flag: every file and all of stdout, byte for byte
    _, plain = run(d, ["-e", EST, "--overlap-ends", "100", "-o", "cb", "reads.fa", "overlaps.paf"])
    assert LINE not in plain and strip_timing("\n".join(out.split("\n")[:-2] + [""])) == strip_timing(plain)
    assert files_of(d, "cb") == sorted(FILES + ENDS)
    for f in FILES + ENDS:
        assert open(d / f"ca.{f}", "rb").read() == open(d / f"cb.{f}", "rb").read(), f


def test_the_option_with_unitigs(dataset):  # noqa: F811
    d = dataset[0]
    args = ["-e", EST, "--overlap-ends", "100", "--best-overlaps", "--unitigs"]
    _, out = run(d, args + ["--containment", "-o", "cu", "reads.fa", "overlaps.paf"])
    want = expected(d, "reads.fa", "overlaps.paf", layout="cu")
    ps = want["placed"]["summary"]
    assert ps["placed"] > ps["n_unitigs"] >= 1 and ps["unitigs_gained"] >= 1 and ps["greatest_depth_permille"] > 1000, ps
    check_run(d, "cu", out, want)
    assert files_of(d, "cu") == sorted(FILES + ENDS + LAYOUT + OURS + DEPTH)
    # the backbone alone is every unitig's own reads: the placed ones are those and the trees below them
    rows = [l.split("\t") for l in want["depth"].decode().splitlines()]
    assert all(int(r[3]) >= int(r[1]) for r in rows) and sum(int(r[3]) for r in rows) == ps["placed"]
    # without the flag: every file and all of stdout, byte for byte
    _, plain = run(d, args + ["-o", "cv", "reads.fa", "overlaps.paf"])
    assert LINE not in plain and PLACE_LINE not in plain and strip_timing("\n".join(out.split("\n")[:-3] + [""])) == strip_timing(plain)
    assert files_of(d, "cv") == sorted(FILES + ENDS + LAYOUT)
    for f in FILES + ENDS + LAYOUT:
        assert open(d / f"cu.{f}", "rb").read() == open(d / f"cv.{f}", "rb").read(), f


@pytest.mark.parametrize("condition", ["filter", "cli_prepare", "two_contexts"])
def test_beside_the_filter_prepared_and_on_two_contexts(dataset, condition):  # noqa: F811
    d = dataset[0]
    extra = ["--min-identity", "99", "--min-overlap", "500"] if condition == "filter" else []
    env = {"cli_prepare": {"RAFT_CLI_PREPARE": "1"}, "two_contexts": {"RAFT_DEVICES": "0,0"}}.get(condition, {})
    prefix = f"c_{condition}"
    _, out = run(d, ["-e", EST] + extra + ["--overlap-ends", "100", "--best-overlaps", "--unitigs", "--containment", "-o", prefix, "reads.fa", "overlaps.paf"], **env)
    keep = None
    if condition == "filter":
        keep = np.array([keeps(l, 990, 500) for l in (d / "overlaps.paf").read_text().splitlines()])
        assert 0 < keep.sum() < keep.size
    want = expected(d, "reads.fa", "overlaps.paf", keep=keep, layout=prefix)
    check_run(d, prefix, out, want)
    if keep is not None:
        assert want["forest"]["summary"]["records"] == int(keep.sum())


def test_beside_every_other_option(dataset):  # noqa: F811
    d = dataset[0]
    every = [a for _, args, _ in ROWS for a in args] + ["--components", "--string-graph"]
    _, out = run(d, ["-e", EST] + every + ["--containment", "-o", "c_all", "reads.fa", "overlaps.paf"])
    got = option_lines(out.split("\n"))
    names = [n for n, _, _ in ROWS]
    at = names.index("unitigs") + 1
    assert [n for n, _ in got] == names[:at] + ["components", "string_graph", "containment", "place_contained"] + names[at:], got
    assert names[at:] == ["fragment_paf"]                 # behind string_graph's, before fragment_paf's
    _, alone = run(d, ["-e", EST, "--overlap-ends", "100", "--best-overlaps", "--unitigs", "--containment", "-o", "c_one", "reads.fa", "overlaps.paf"])
    assert [dict(got)["containment"], dict(got)["place_contained"]] == alone.split("\n")[-3:-1]
    theirs = tuple(f for _, _, fs in ROWS for f in fs) + ("components.tsv", "components.summary.tsv", "string_graph.gfa", "string_graph.tsv")
    assert files_of(d, "c_all") == sorted(FILES + theirs + OURS + DEPTH)
    for f in OURS + DEPTH:
        assert open(d / f"c_all.{f}", "rb").read() == open(d / f"c_one.{f}", "rb").read(), f
    check_run(d, "c_one", alone, expected(d, "reads.fa", "overlaps.paf", layout="c_one"))
    # ... and the other options' files and lines are those of the run without the flag
    _, without = run(d, ["-e", EST] + every + ["-o", "c_none", "reads.fa", "overlaps.paf"])
    ours = lambda l: l.startswith(LINE) or l.startswith(PLACE_LINE)
    assert [l for l in out.split("\n") if not ours(l) and not l.startswith(CMD) and "program completed after" not in l] == \
           [l for l in without.split("\n") if not l.startswith(CMD) and "program completed after" not in l]
    assert files_of(d, "c_none") == sorted(FILES + theirs)
    for f in files_of(d, "c_none"):
        assert open(d / f"c_all.{f}", "rb").read() == open(d / f"c_none.{f}", "rb").read(), f


@pytest.mark.parametrize("args", [["--containment"], ["--overlap-ends", "100", "--containment", "--unitigs"]],
                         ids=["without --overlap-ends", "--unitigs without --best-overlaps"])
def test_the_usage_errors(dataset, args):  # noqa: F811
    d = dataset[0]
    rc, out = run(d, ["-e", EST] + args + ["-o", "c_bad", "reads.fa", "overlaps.paf"], ok=False)
    assert rc == 1 and "Usage: raft [options] <input-reads.fa> <in.paf>" in out and "ERROR" not in out
    assert files_of(d, "c_bad") == []


def test_the_two_step_recipe_on_the_fragments(dataset):  # noqa: F811
    d = dataset[0]
    run(d, ["-e", EST, "--fragment-paf", "-o", "cf", "reads.fa", "overlaps.paf"])
    _, out = run(d, ["-e", "20", "--overlap-ends", "100", "--best-overlaps", "--unitigs", "--containment", "-o", "cf2", "cf.reads.fasta", "cf.fragments.paf"])
    want = expected(d, "cf.reads.fasta", "cf.fragments.paf", layout="cf2")
    check_run(d, "cf2", out, want)
    assert want["forest"]["summary"]["reads_with_parent"] >= 1 and len(want["names"]) > 300
