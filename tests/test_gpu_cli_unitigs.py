"""GPU: `raft --overlap-ends H --best-overlaps --unitigs` -- PREFIX.unitigs.tsv, PREFIX.unitigs.layout.tsv and the option's stdout line
against the sequential walk of tests/unitig_testlib.py over the numpy restatements of overlap_ends and best_overlaps on
``hostio.load_paf(strand=True)``; every other file and the rest of stdout byte for byte those of a run without the flag.  The test
writes its own set: reads tiled along a line with dovetail overlaps on both strands (one long chain), a small circle, a contained read
and an isolated one."""
import os

import numpy as np
import pytest
from raft_testlib import write_fasta
from test_gpu_best_overlaps import want_best
from test_gpu_cli_filter import keeps
from test_gpu_cli_overlap_ends import CMD, FILES, FILTER_LINE, files_of, run, strip_timing
from test_gpu_overlap_ends import want_all
from unitig_testlib import files_of as unitig_files
from unitig_testlib import stdout_line, walk

from raft_amd import hostio

pytestmark = pytest.mark.gpu
LINE = "INFO, unitigs(), "
BEST_LINE = "INFO, best_overlaps(), "
NEW = ("overlap_ends.tsv", "best_overlaps.tsv")
OURS = ("unitigs.layout.tsv", "unitigs.tsv")
CHAIN, CIRCLE, LEN, STEP = 40, 4, 5000, 3000


def paf_line(names, rl, a, b, a_range, b_range, rev, matches=None):
    block = max(a_range[1] - a_range[0], b_range[1] - b_range[0]) + 3
    return "\t".join([names[a], str(rl[a]), str(a_range[0]), str(a_range[1]), "+-"[rev], names[b], str(rl[b]), str(b_range[0]), str(b_range[1]),
                      str(block * 995 // 1000 if matches is None else matches), str(block), "60"])


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """Reads 0 .. CHAIN - 1 tile a line every STEP bases, each on a strand of its own; CIRCLE more tile a circle; one lies inside read 5; one has no overlap."""
    d = tmp_path_factory.mktemp("unitigs_cli")
    rng = np.random.default_rng(7)
    n = CHAIN + CIRCLE + 2
    contained = CHAIN + CIRCLE                                            # (the read behind it has no overlap)
    rl = np.full(n, LEN, np.int32)
    rl[:CHAIN] += rng.integers(0, 400, CHAIN).astype(np.int32)            # (tails of different lengths: spans that differ)
    rl[contained] = 1000
    order = rng.permutation(n)                                            # the ids of the file are not those of the layout
    names = [f"r{order[i]}" for i in range(n)]
    back = rng.integers(0, 2, n)                                          # 1: the read is the reverse complement of its stretch
    back[0], back[1], back[2] = 0, 1, 1
    pairs = []                                                            # (a, b, the bases of a's stretch behind which b begins, the overlap)
    for i in range(CHAIN - 1):
        pairs.append((i, i + 1, STEP, int(rl[i]) - STEP))
    for j in range(CIRCLE):
        pairs.append((CHAIN + j, CHAIN + (j + 1) % CIRCLE, STEP, LEN - STEP))
    lines = []
    for a, b, at, ovl in pairs:
        a_range = (at, at + ovl) if not back[a] else (int(rl[a]) - at - ovl, int(rl[a]) - at)
        b_range = (0, ovl) if not back[b] else (int(rl[b]) - ovl, int(rl[b]))
        rev = int(back[a] != back[b])
        weak = 900 * (ovl + 3) // 1000 if a == 20 else None               # one overlap of the chain below 99 % identity
        lines.append((a, paf_line(names, rl, a, b, a_range, b_range, rev, weak)))
        lines.append((b, paf_line(names, rl, b, a, b_range, a_range, rev, weak)))
    lines.append((contained, paf_line(names, rl, contained, 5, (0, 1000), (2000, 3000), 0)))
    lines.append((5, paf_line(names, rl, 5, contained, (2000, 3000), (0, 1000), 0)))
    lines.sort(key=lambda x: x[0])
    write_fasta(d / "reads.fa", names, rl)
    (d / "overlaps.paf").write_text("".join(l + "\n" for _, l in lines))
    return d, names, rl


def expected(d, names, rl, H=1000, F=800, keep=None):
    """-> the texts of the two files, the stdout line and the walk's result, from the restatements over the tokenised file"""
    reads = hostio.Reads(str(d / "reads.fa"))
    cols, sym = hostio.load_paf(str(d / "overlaps.paf"), reads, with_flag=True, strand=True)
    reads.close()
    if keep is not None:
        cols = [c[keep(cols)] for c in cols]
    status = want_all(rl, cols[:6], cols[6], H, F, bool(sym))[2]
    partner, span, flags, _ = want_best(rl, cols[:6], cols[6], H, F, bool(sym), (status == 1).astype("uint8"))
    w = walk(rl, partner, span, flags)
    table, layout = unitig_files(w, names, rl)
    return table.encode(), layout.encode(), stdout_line(w), w


def test_the_set_holds_a_chain_a_circle_a_contained_and_an_isolated_read(dataset):
    d, names, rl = dataset
    _, _, line, w = expected(d, names, rl)
    s = w["summary"]
    assert (s["reads_in"], s["reads_skipped"], s["unitigs"], s["singletons"], s["circular"], s["longest_reads"]) == (CHAIN + CIRCLE + 2, 1, 3, 1, 1, CHAIN), s
    assert 0 < int(w["orient"].sum()) < CHAIN and line.startswith(LINE)
    assert sorted(w["utg_reads"]) == [1, CIRCLE, CHAIN] and s["longest_length"] == (CHAIN - 1) * STEP + int(rl[CHAIN - 1])
    assert w["utg_length"][np.flatnonzero(w["utg_circular"])[0]] == CIRCLE * STEP


def test_the_files_and_the_line_equal_the_walk(dataset):
    d, names, rl = dataset
    opts = ["-e", "20", "--overlap-ends", "1000", "--best-overlaps"]
    rc, plain = run(d, opts + ["-o", "b", "reads.fa", "overlaps.paf"])
    assert rc == 0 and LINE not in plain and BEST_LINE in plain, plain
    rc, out = run(d, opts + ["--unitigs", "-o", "a", "reads.fa", "overlaps.paf"])
    assert rc == 0, out
    want_table, want_layout, want_line, _ = expected(d, names, rl)
    lines = out.split("\n")
    assert lines[-1] == "" and lines[-2] == want_line and lines[-3].startswith(BEST_LINE) and sum(l.startswith(LINE) for l in lines) == 1, lines[-4:]
    # without the flag: stdout and every other file, byte for byte
    assert strip_timing("\n".join(lines[:-2] + [""])) == strip_timing(plain)
    assert files_of(d, "b") == sorted(FILES + NEW) and files_of(d, "a") == sorted(FILES + NEW + OURS)
    for f in files_of(d, "b"):
        assert open(d / f"a.{f}", "rb").read() == open(d / f"b.{f}", "rb").read(), f
    assert open(d / "a.unitigs.tsv", "rb").read() == want_table
    assert open(d / "a.unitigs.layout.tsv", "rb").read() == want_layout


def test_behind_the_filter_the_weak_overlap_breaks_the_chain(dataset):
    d, names, rl = dataset
    rc, out = run(d, ["-e", "20", "--min-identity", "99", "--overlap-ends", "1000", "--best-overlaps", "--unitigs", "-o", "f", "reads.fa", "overlaps.paf"])
    assert rc == 0, out
    lines = out.split("\n")
    at = [i for i, l in enumerate(lines) if l.startswith(FILTER_LINE)]
    assert len(at) == 1 and lines[at[0] - 1].startswith(CMD)
    kept = np.array([keeps(l, 990, 0) for l in (d / "overlaps.paf").read_text().splitlines()])
    assert kept.sum() == kept.size - 2 and f", kept = {int(kept.sum())}," in lines[at[0]]
    want_table, want_layout, want_line, w = expected(d, names, rl, keep=lambda cols: kept)
    assert lines[-2] == want_line and sorted(w["utg_reads"]) == [1, CIRCLE, CHAIN - 21, 21]
    assert open(d / "f.unitigs.tsv", "rb").read() == want_table
    assert open(d / "f.unitigs.layout.tsv", "rb").read() == want_layout


@pytest.mark.parametrize("bad", [["--unitigs"], ["--overlap-ends", "1000", "--unitigs"], ["--overlap-ends", "1000", "--best-overlaps", "--unitigs=1"],
                                 ["--unitigs=1"]], ids=lambda b: " ".join(b))
def test_the_flag_without_best_overlaps_or_with_a_value_is_the_usage_error(tmp_path, bad):
    rc, out = run(tmp_path, ["-e", "3"] + bad + ["reads.fa", "overlaps.paf"])
    assert rc == 1 and "Usage: raft [options] <input-reads.fa> <in.paf>\n" in out, out
    assert os.listdir(tmp_path) == []
