"""GPU: `raft --fragment-paf [--fragment-paf-min L]` -- PREFIX.fragments.paf and the option's stdout line against the writer's bytes
over the brute-force oracle's lift (tests/lift_testlib.py) of the tokenised stream onto the fragment table read back from
PREFIX.reads.fasta; the four reference files and the rest of stdout byte for byte those of a run without the flag; a second
`raft --overlap-ends --best-overlaps --unitigs` on PREFIX.reads.fasta and PREFIX.fragments.paf runs through and sees as many records as
were lifted; the same beside --min-overlap (where fields 10 and 11 are scaled from the source's) and on two contexts."""
import os
import re

import numpy as np
import pytest
from lift_testlib import lift
from raft_testlib import write_fasta
from test_gpu_cli_filter import keeps
from test_gpu_cli_overlap_ends import CMD, FILES, FILTER_LINE, files_of, run, strip_timing

from raft_amd import hostio

pytestmark = pytest.mark.gpu
LINE = "INFO, fragment_paf(), "
ENDS_LINE = "INFO, overlap_ends(), "
OURS = ("fragments.paf",)
EST = "30"                              # (under -e 30 the pass cuts three reads of the set into three fragments)


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """300 reads at 30-fold coverage, both strands, fields 10 and 11 between 97.5 and 100 %: a pass under -e 30 cuts reads into two
    and three fragments."""
    from raft_amd.synth import make_overlaps
    d = tmp_path_factory.mktemp("lift_cli")
    o = make_overlaps(300, coverage=30, seed=5)
    rl = o.read_len.numpy()
    qid, qs, qe, tid, ts, te = (c.numpy().astype(np.int64) for c in o.columns())
    names = [f"r{i}" for i in range(o.n_reads)]
    write_fasta(d / "reads.fa", names, rl)
    pair = (np.minimum(qid, tid) * 2 ** 20 + np.maximum(qid, tid)) * 7919 + 13          # (a record and its mirror agree)
    rev = (pair // 41) % 2
    block = np.maximum(qe - qs, te - ts) + 3
    matches = -(-block * (975 + pair % 26) // 1000)
    lines = ["\t".join([names[qid[i]], str(rl[qid[i]]), str(qs[i]), str(qe[i]), "+-"[rev[i]], names[tid[i]], str(rl[tid[i]]), str(ts[i]), str(te[i]),
                        str(matches[i]), str(block[i]), "60"]) for i in range(qid.size)]
    (d / "overlaps.paf").write_text("".join(l + "\n" for l in lines))
    return d, names, rl


def table_of(d, prefix, names):
    """The fragment table PREFIX.reads.fasta was written from, read back from its headers."""
    index = {n: i for i, n in enumerate(names)}
    rows = [[] for _ in names]
    at = 0
    for ln in open(d / f"{prefix}.reads.fasta"):
        if ln.startswith(">"):
            m = re.fullmatch(r">read=(\d+),(\w+),pos_on_original_read=(\d+)-(\d+)\n", ln)
            at += 1
            assert m and int(m.group(1)) == at, ln
            rows[index[m.group(2)]].append((at - 1, int(m.group(3)), int(m.group(4))))
    flat = [r for per in rows for r in per]
    assert [r[0] for r in flat] == list(range(at))                      # rows in read order
    off = np.concatenate([[0], np.cumsum([len(per) for per in rows])]).astype(np.int64)
    return off, np.array([r[1] for r in flat], np.int32), np.array([r[2] for r in flat], np.int32)


def expected(d, prefix, names, min_len=1, keep=None):
    """-> the bytes of PREFIX.fragments.paf, the stdout line and the oracle's result, for the run that wrote PREFIX.reads.fasta"""
    table = table_of(d, prefix, names)
    reads = hostio.Reads(str(d / "reads.fa"))
    try:
        cols = hostio.load_paf(str(d / "overlaps.paf"), reads, quality=keep is not None, strand=True)
        if keep is not None:
            cols = [c[keep] for c in cols]
        res = lift(*table, cols[:6], cols[-1], min_len)
        quality = (cols[6], cols[7]) if keep is not None else (None, None)
        hostio.write_fragment_paf(str(d / f"want_{prefix}.paf"), reads, table, res, *quality)
    finally:
        reads.close()
    line = (f"{LINE}min_len = {min_len}, records = {res['n_records']}, lifted = {res['n_out']}, cut = {res['records_cut']}, "
            f"without a fragment pair = {res['records_none']}, dropped pairs = {res['pairs_dropped']}, most from one record = {res['most_per_record']}")
    return open(d / f"want_{prefix}.paf", "rb").read(), line, res, table


def second_run(d, prefix, lifted):
    """The fragments as a read set of their own: the same questions asked again, without another overlapper run."""
    rc, out = run(d, ["-e", "20", "--overlap-ends", "100", "--best-overlaps", "--unitigs", "-o", prefix + "2", f"{prefix}.reads.fasta", f"{prefix}.fragments.paf"])
    assert rc == 0, out
    ends = [l for l in out.split("\n") if l.startswith(ENDS_LINE)]
    assert len(ends) == 1 and f", records = {lifted}," in ends[0], ends
    assert "INFO, unitigs(), " in out and os.path.getsize(d / f"{prefix}2.unitigs.tsv") > 0


def test_the_file_and_the_line_equal_the_oracle_and_the_loop_closes(dataset):
    d, names, rl = dataset
    rc, plain = run(d, ["-e", EST, "-o", "b", "reads.fa", "overlaps.paf"])
    assert rc == 0 and LINE not in plain, plain
    rc, out = run(d, ["-e", EST, "--fragment-paf", "-o", "a", "reads.fa", "overlaps.paf"])
    assert rc == 0, out
    want_file, want_line, res, table = expected(d, "a", names)
    assert np.diff(table[0]).max() >= 3 and res["records_cut"] > 0 and res["n_out"] > res["n_records"] // 2
    lines = out.split("\n")
    assert lines[-1] == "" and lines[-2] == want_line and sum(l.startswith(LINE) for l in lines) == 1, (lines[-3:], want_line)
    # without the flag: stdout and the four reference files, byte for byte
    assert strip_timing("\n".join(lines[:-2] + [""])) == strip_timing(plain)
    assert files_of(d, "b") == sorted(FILES) and files_of(d, "a") == sorted(FILES + OURS)
    for f in FILES:
        assert open(d / f"a.{f}", "rb").read() == open(d / f"b.{f}", "rb").read(), f
    got = open(d / "a.fragments.paf", "rb").read()
    assert got == want_file and got.count(b"\n") == res["n_out"]
    second_run(d, "a", res["n_out"])


def test_the_minimum_length(dataset):
    d, names, rl = dataset
    rc, out = run(d, ["-e", EST, "--fragment-paf", "--fragment-paf-min", "501", "-o", "m", "reads.fa", "overlaps.paf"])
    assert rc == 0, out
    want_file, want_line, res, _ = expected(d, "m", names, min_len=501)
    assert out.split("\n")[-2] == want_line and res["pairs_dropped"] > 0
    assert open(d / "m.fragments.paf", "rb").read() == want_file


def test_beside_the_filter(dataset):
    """The kept stream is what is lifted, and fields 10 and 11 are scaled from the kept records' own."""
    d, names, rl = dataset
    rc, plain = run(d, ["-e", EST, "--min-identity", "99", "--min-overlap", "500", "-o", "fb", "reads.fa", "overlaps.paf"])
    assert rc == 0, plain
    rc, out = run(d, ["-e", EST, "--min-identity", "99", "--min-overlap", "500", "--fragment-paf", "-o", "fa", "reads.fa", "overlaps.paf"])
    assert rc == 0, out
    kept = np.array([keeps(l, 990, 500) for l in (d / "overlaps.paf").read_text().splitlines()])
    assert 0 < kept.sum() < kept.size
    want_file, want_line, res, _ = expected(d, "fa", names, keep=kept)
    lines = out.split("\n")
    at = [i for i, l in enumerate(lines) if l.startswith(FILTER_LINE)]
    assert len(at) == 1 and lines[at[0] - 1].startswith(CMD) and f", kept = {int(kept.sum())}," in lines[at[0]]
    assert lines[-2] == want_line and res["n_records"] == int(kept.sum())
    assert strip_timing("\n".join(lines[:-2] + [""])) == strip_timing(plain)
    for f in FILES:
        assert open(d / f"fa.{f}", "rb").read() == open(d / f"fb.{f}", "rb").read(), f
    got = open(d / "fa.fragments.paf", "rb").read()
    assert got == want_file
    # (scaled: a line's field 10 is below its smaller span somewhere)
    fields = [l.split(b"\t") for l in got.split(b"\n")[:-1]]
    assert any(int(f[9]) < min(int(f[3]) - int(f[2]), int(f[8]) - int(f[7])) for f in fields)
    second_run(d, "fa", res["n_out"])


def test_on_two_contexts(dataset):
    d, names, rl = dataset
    rc, out = run(d, ["-e", EST, "--fragment-paf", "-o", "d", "reads.fa", "overlaps.paf"], RAFT_DEVICES="0,0")
    assert rc == 0, out
    want_file, want_line, res, _ = expected(d, "d", names)
    assert out.split("\n")[-2] == want_line
    assert open(d / "d.fragments.paf", "rb").read() == want_file
    second_run(d, "d", res["n_out"])
