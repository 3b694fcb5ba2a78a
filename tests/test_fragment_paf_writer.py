"""CPU: raft_host_write_fragment_paf (include/raft_host_lift.h) -- the bytes of PREFIX.fragments.paf on a small table stated by hand,
for both header forms (real and simulated reads); the names equal to the first words of the headers of a reads.fasta that
raft_host_write_fasta wrote for the same table, read back; both forms of fields 10 and 11; the same bytes under 1 and 4 threads; a row
outside the table, columns of other lengths or an unwritable path are refused."""
import numpy as np
import pytest
from lift_testlib import COLUMNS, lift, make_stream
from raft_testlib import write_fasta

from raft_amd import hostio
from raft_amd.hostio import ptr

REAL = ["r0/x", "r1/x", "r2/x", "r3/x"]
SIMULATED = ["read=1,forward,position=1000-3000,length=2000,chr1", "read=2,reverse,position=500-3500,length=3000,chr1",
             "read=3,forward,position=0-800,length=800,chr2", "read=4,reverse,position=10-2510,length=2500,chr2"]
LENGTHS = [2000, 3000, 800, 2500]
# read 0: two fragments, read 1: three, read 2: one (whole), read 3: two
OFF = np.array([0, 2, 5, 6, 8], np.int64)
FB = np.array([0, 900, 0, 1000, 1900, 0, 0, 1200], np.int32)
FE = np.array([1400, 2000, 1500, 2400, 3000, 800, 1700, 2500], np.int32)
TABLE = (OFF, FB, FE)


@pytest.fixture(autouse=True)
def default_threads():
    yield
    hostio.set_threads(0)


def load(tmp_path, names):
    write_fasta(tmp_path / "in.fa", names, LENGTHS)
    return hostio.Reads(str(tmp_path / "in.fa"))


def fasta_names(tmp_path, reads):
    """The first word of every header of the reads.fasta raft_host_write_fasta writes for TABLE, by row."""
    path = tmp_path / "out.reads.fasta"
    assert hostio.load_library().raft_host_write_fasta(str(path).encode(), reads._h, ptr(OFF), ptr(FB), ptr(FE)) == hostio.OK
    heads = [ln[1:] for ln in path.read_text().split("\n") if ln.startswith(">")]
    assert len(heads) == FB.size
    return [h.split()[0] for h in heads], heads


def expected(names, res, matches=None, block=None):
    """The file, formatted here."""
    out = []
    flen = (FE - FB).tolist()
    for k in range(res["qfrag"].size):
        q, t = int(res["qfrag"][k]), int(res["tfrag"][k])
        sq, st = int(res["qe"][k]) - int(res["qs"][k]), int(res["te"][k]) - int(res["ts"][k])
        big, small = max(sq, st), min(sq, st)
        if matches is not None:
            s = int(res["src"][k])
            small = 0 if block[s] <= 0 else min(big, max(int(matches[s]), 0) * big // int(block[s]))
        out.append("\t".join(str(x) for x in (names[q], flen[q], res["qs"][k], res["qe"][k], "-" if res["rev"][k] else "+", names[t], flen[t],
                                                res["ts"][k], res["te"][k], small, big, 255)) + "\n")
    return "".join(out).encode()


def columns(rows):
    """rows of (qfrag, qs, qe, tfrag, ts, te, rev, src) -> the dict Engine.lift_overlaps returns"""
    a = np.asarray(rows, np.int64).reshape(-1, 8)
    return {k: a[:, i].astype(np.uint8 if k == "rev" else np.int32) for i, k in enumerate(COLUMNS)}


ROWS = [(0, 100, 400, 2, 50, 350, 0, 0), (1, 0, 1100, 4, 0, 1000, 1, 1), (5, 0, 800, 7, 500, 1300, 0, 2), (3, 10, 20, 6, 1690, 1700, 1, 2)]


def test_the_bytes_of_a_small_table_real_reads(tmp_path):
    reads = load(tmp_path, REAL)
    try:
        hostio.write_fragment_paf(str(tmp_path / "x.fragments.paf"), reads, TABLE, columns(ROWS))
        names, heads = fasta_names(tmp_path, reads)
    finally:
        reads.close()
    assert (tmp_path / "x.fragments.paf").read_text() == (
        "read=1,r0/x,pos_on_original_read=0-1400\t1400\t100\t400\t+\tread=3,r1/x,pos_on_original_read=0-1500\t1500\t50\t350\t300\t300\t255\n"
        "read=2,r0/x,pos_on_original_read=900-2000\t1100\t0\t1100\t-\tread=5,r1/x,pos_on_original_read=1900-3000\t1100\t0\t1000\t1000\t1100\t255\n"
        "read=6,r2/x,pos_on_original_read=0-800\t800\t0\t800\t+\tread=8,r3/x,pos_on_original_read=1200-2500\t1300\t500\t1300\t800\t800\t255\n"
        "read=4,r1/x,pos_on_original_read=1000-2400\t1400\t10\t20\t-\tread=7,r3/x,pos_on_original_read=0-1700\t1700\t1690\t1700\t10\t10\t255\n")
    assert names == heads and names[4] == "read=5,r1/x,pos_on_original_read=1900-3000"


def test_the_bytes_of_a_small_table_simulated_reads(tmp_path):
    reads = load(tmp_path, SIMULATED)
    try:
        hostio.write_fragment_paf(str(tmp_path / "x.fragments.paf"), reads, TABLE, columns(ROWS))
        names, heads = fasta_names(tmp_path, reads)
    finally:
        reads.close()
    # forward: position = start + [b, e); reverse: end - [e, b); a read kept whole keeps its own position and length
    assert names == ["read=1,forward,position=1000-2400,length=1400,chr1", "read=2,forward,position=1900-3000,length=1100,chr1",
                     "read=3,reverse,position=2000-3500,length=1500,chr1", "read=4,reverse,position=1100-2500,length=1400,chr1",
                     "read=5,reverse,position=500-1600,length=1100,chr1", "read=6,forward,position=0-800,length=800,chr2",
                     "read=7,reverse,position=810-2510,length=1700,chr2", "read=8,reverse,position=10-1310,length=1300,chr2"] == heads
    lines = (tmp_path / "x.fragments.paf").read_text().split("\n")
    assert lines[0] == f"{names[0]}\t1400\t100\t400\t+\t{names[2]}\t1500\t50\t350\t300\t300\t255"
    assert lines[3] == f"{names[3]}\t1400\t10\t20\t-\t{names[6]}\t1700\t1690\t1700\t10\t10\t255" and lines[4] == ""
    assert (tmp_path / "x.fragments.paf").read_bytes() == expected(names, columns(ROWS))


@pytest.mark.parametrize("form", ["real", "simulated"])
@pytest.mark.parametrize("threads", [1, 4])
def test_a_lifted_stream_under_both_forms_of_fields_10_and_11(tmp_path, form, threads):
    """The oracle's lift of a random stream: names equal to the first words of reads.fasta's headers, read back; the same bytes
    whatever the thread count."""
    hostio.set_threads(threads)
    rng = np.random.default_rng(21)
    cols, strand = make_stream(rng, np.array(LENGTHS, np.int32), 9000)
    res = lift(OFF, FB, FE, cols, strand)
    assert res["n_out"] > 9000 and res["records_cut"] > 0
    matches = rng.integers(-5, 3000, 9000).astype(np.int32)
    block = rng.integers(-5, 3000, 9000).astype(np.int32)
    matches[:3], block[:3] = (2 ** 31 - 1, 7, 0), (1, 0, 0)
    reads = load(tmp_path, REAL if form == "real" else SIMULATED)
    try:
        names, _ = fasta_names(tmp_path, reads)
        hostio.write_fragment_paf(str(tmp_path / "plain.paf"), reads, TABLE, res)
        hostio.write_fragment_paf(str(tmp_path / "scaled.paf"), reads, TABLE, res, matches, block)
    finally:
        reads.close()
    assert (tmp_path / "plain.paf").read_bytes() == expected(names, res)
    scaled = (tmp_path / "scaled.paf").read_bytes()
    assert scaled == expected(names, res, matches, block) and scaled != (tmp_path / "plain.paf").read_bytes()
    fields = [ln.split("\t") for ln in scaled.decode().split("\n")[:-1]]
    assert len(fields) == res["n_out"] and all(len(f) == 12 and 0 <= int(f[9]) <= int(f[10]) and f[11] == "255" for f in fields)
    assert all(int(f[3]) <= int(f[1]) and int(f[8]) <= int(f[6]) for f in fields)


def test_no_outputs(tmp_path):
    reads = load(tmp_path, REAL)
    try:
        hostio.write_fragment_paf(str(tmp_path / "e.paf"), reads, TABLE, columns([]))
    finally:
        reads.close()
    assert (tmp_path / "e.paf").read_bytes() == b""


def test_the_refusals(tmp_path):
    reads = load(tmp_path, REAL)
    try:
        for bad_row in (8, -1, 2 ** 31 - 1):
            for col in (0, 3):
                rows = [list(r) for r in ROWS]
                rows[2][col] = bad_row
                with pytest.raises(hostio.HostError):
                    hostio.write_fragment_paf(str(tmp_path / "y.paf"), reads, TABLE, columns(rows))
        assert not (tmp_path / "y.paf").exists()
        res = columns(ROWS)
        with pytest.raises(ValueError):
            hostio.write_fragment_paf(str(tmp_path / "y.paf"), reads, TABLE, {**res, "rev": res["rev"][:-1]})
        with pytest.raises(ValueError):
            hostio.write_fragment_paf(str(tmp_path / "y.paf"), reads, (OFF[:-1], FB, FE), res)
        with pytest.raises(ValueError):
            hostio.write_fragment_paf(str(tmp_path / "y.paf"), reads, TABLE, res, np.ones(3, np.int32))
        with pytest.raises(ValueError):
            hostio.write_fragment_paf(str(tmp_path / "y.paf"), reads, TABLE, res, np.ones(2, np.int32), np.ones(2, np.int32))     # src 2 points behind
        with pytest.raises(hostio.HostError):
            hostio.write_fragment_paf(str(tmp_path / "no" / "such" / "dir.paf"), reads, TABLE, res)
    finally:
        reads.close()
