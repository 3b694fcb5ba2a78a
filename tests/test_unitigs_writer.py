"""CPU: raft_host_write_unitigs (include/raft_host_utg.h) -- the bytes of PREFIX.unitigs.tsv and PREFIX.unitigs.layout.tsv on a table
with a path, a cycle, a singleton and a skipped read, stated by hand and equal to a Python format; larger tables; no unitigs; a table
that names a read outside the set, whose offsets do not ascend, or an unwritable path are refused."""
import numpy as np
import pytest
from raft_testlib import write_fasta
from test_host_paf_quality import N_READS, NAMES
from unitig_testlib import files_of, make_table, walk

from raft_amd import hostio

LENGTHS = [50 + i for i in range(N_READS)]


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    d = tmp_path_factory.mktemp("utg_reads")
    write_fasta(d / "reads.fa", NAMES, LENGTHS)
    r = hostio.Reads(str(d / "reads.fa"))
    yield r
    r.close()
    hostio.set_threads(0)


def test_a_path_a_cycle_a_singleton_and_a_skipped_read(tmp_path):
    """Seven reads: 5 -> 0 -> 3 on one strand (the start is 3, so all are '-'), the cycle 1 -> 6 with 6 reversed, 2 alone, 4 left out"""
    names, lens = [f"r{i}/x" for i in range(7)], [1000, 2000, 300, 4000, 77, 6000, 7000]
    write_fasta(tmp_path / "reads.fa", names, lens)
    partner, span, flags = np.full((7, 2), -1, np.int32), np.zeros((7, 2), np.int32), np.zeros(7, np.uint8)
    for a, ea, b, eb, s in ((5, 1, 0, 0, 100), (0, 1, 3, 0, 200), (1, 1, 6, 1, 10), (6, 0, 1, 0, 20)):
        rev = 1 if ea == eb else 0
        for r, e, p in ((a, ea, b), (b, eb, a)):
            partner[r, e], span[r, e] = p, s
            flags[r] |= (2 | rev) << (2 * e)
    flags[4] = 16
    w = walk(np.array(lens, np.int32), partner, span, flags)
    reads = hostio.Reads(str(tmp_path / "reads.fa"))
    try:
        hostio.write_unitigs(str(tmp_path / "x"), reads, w)
    finally:
        reads.close()
    assert (tmp_path / "x.unitigs.tsv").read_text() == ("0\t2\t8970\t1\tr1/x\tr6/x\n"
                                                        "1\t1\t300\t0\tr2/x\tr2/x\n"
                                                        "2\t3\t10700\t0\tr3/x\tr5/x\n")
    assert (tmp_path / "x.unitigs.layout.tsv").read_text() == ("0\t0\tr1/x\t2000\t+\t0\n"
                                                               "0\t1\tr6/x\t7000\t-\t1990\n"
                                                               "1\t0\tr2/x\t300\t+\t0\n"
                                                               "2\t0\tr3/x\t4000\t-\t0\n"
                                                               "2\t1\tr0/x\t1000\t-\t3800\n"
                                                               "2\t2\tr5/x\t6000\t-\t4700\n")
    assert sorted(p.name for p in tmp_path.iterdir()) == ["reads.fa", "x.unitigs.layout.tsv", "x.unitigs.tsv"]


@pytest.mark.parametrize("threads", [1, 7])
def test_the_writer_equals_a_python_format(tmp_path, reads, threads):
    hostio.set_threads(threads)
    rng = np.random.default_rng(12)
    L, partner, span, flags = make_table(rng, N_READS, [(9, False), (5, True), (2, True), (3, False)], skipped=6, len_range=(10, 50))
    L = np.array(LENGTHS, np.int32)                                    # (the reads' own lengths: spans of at most 50 fit every read)
    w = walk(L, partner, span, flags)
    w["offset"][w["order"][-1]] = 2 ** 62 + 5                          # (the writer prints what it is given)
    w["utg_length"][0] = 2 ** 62 + 7
    hostio.write_unitigs(str(tmp_path / "y"), reads, w)
    table, layout = files_of(w, NAMES, L)
    assert (tmp_path / "y.unitigs.tsv").read_bytes() == table.encode() and (tmp_path / "y.unitigs.layout.tsv").read_bytes() == layout.encode()
    assert table.count("\n") == w["summary"]["unitigs"] and layout.count("\n") == N_READS - 6
    assert all(len(l.split("\t")) == 6 for l in (table + layout).split("\n")[:-1])
    assert "\t+\t" in layout and "\t-\t" in layout and str(2 ** 62 + 5) in layout and str(2 ** 62 + 7) in table


def test_no_unitigs(tmp_path, reads):
    (tmp_path / "empty.fa").write_text("")
    r = hostio.Reads(str(tmp_path / "empty.fa"))
    try:
        assert r.n == 0
        hostio.write_unitigs(str(tmp_path / "e"), r, walk(np.zeros(0, np.int32), np.zeros((0, 2), np.int32), np.zeros((0, 2), np.int32), np.zeros(0, np.uint8)))
        assert (tmp_path / "e.unitigs.tsv").read_bytes() == b"" and (tmp_path / "e.unitigs.layout.tsv").read_bytes() == b""
    finally:
        r.close()
    # every read left out: no unitigs either
    n = N_READS
    w = walk(np.array(LENGTHS, np.int32), np.full((n, 2), -1, np.int32), np.zeros((n, 2), np.int32), np.full(n, 16, np.uint8))
    hostio.write_unitigs(str(tmp_path / "s"), reads, w)
    assert (tmp_path / "s.unitigs.tsv").read_bytes() == b"" and (tmp_path / "s.unitigs.layout.tsv").read_bytes() == b""


def test_the_refusals(tmp_path, reads):
    rng = np.random.default_rng(3)
    L, partner, span, flags = make_table(rng, N_READS, [(9, False), (5, True)], skipped=6, len_range=(10, 50))
    sound = walk(np.array(LENGTHS, np.int32), partner, span, flags)
    for key in ("unitig", "offset", "orient", "utg_reads", "utg_circular", "order"):
        w = dict(sound)
        w[key] = w[key][:-1]
        with pytest.raises(ValueError):
            hostio.write_unitigs(str(tmp_path / "y"), reads, w)
    for bad in (N_READS, -1, 2 ** 31 - 1):
        w = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in sound.items()}
        w["order"][3] = bad
        with pytest.raises(hostio.HostError):
            hostio.write_unitigs(str(tmp_path / "y"), reads, w)
    w = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in sound.items()}
    w["utg_off"][1] = w["utg_off"][2]                                  # a unitig without reads
    with pytest.raises(hostio.HostError):
        hostio.write_unitigs(str(tmp_path / "y"), reads, w)
    w["utg_off"][:] = sound["utg_off"] + 1                             # does not begin at 0
    w["order"] = np.append(w["order"], 0).astype(np.int32)
    with pytest.raises(hostio.HostError):
        hostio.write_unitigs(str(tmp_path / "y"), reads, w)
    assert not (tmp_path / "y.unitigs.tsv").exists() and not (tmp_path / "y.unitigs.layout.tsv").exists()
    with pytest.raises(hostio.HostError):
        hostio.write_unitigs(str(tmp_path / "no" / "such" / "dir"), reads, sound)
