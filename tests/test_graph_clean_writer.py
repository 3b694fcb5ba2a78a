"""CPU: raft_host_write_graph_clean (include/raft_host_cln.h) -- the bytes of PREFIX.clean.tsv on a literal table, stated by hand, with
1 and 7 workers; a larger table against a Python format; no reads; a state outside the three, a negative count, arrays of the wrong
length or an unwritable path is refused."""
import numpy as np
import pytest
from raft_testlib import write_fasta
from test_host_paf_quality import N_READS, NAMES

from raft_amd import hostio

LENGTHS = [50 + i for i in range(N_READS)]
STATES = ("kept", "tip", "flagged")


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    d = tmp_path_factory.mktemp("cln_reads")
    write_fasta(d / "reads.fa", NAMES, LENGTHS)
    r = hostio.Reads(str(d / "reads.fa"))
    yield r
    r.close()
    hostio.set_threads(0)


def clean_text(names, lens, res):
    """PREFIX.clean.tsv as include/raft_host_cln.h has it: name length state round weak5 kept5 weak3 kept3"""
    weak, kept = np.asarray(res["weak"]).reshape(-1, 2), np.asarray(res["kept"]).reshape(-1, 2)
    return "".join(f"{name}\t{lens[i]}\t{STATES[res['read_state'][i]]}\t{res['read_round'][i]}\t{weak[i, 0]}\t{kept[i, 0]}\t{weak[i, 1]}\t{kept[i, 1]}\n"
                   for i, name in enumerate(names))


LITERAL = dict(read_state=np.array([0, 1, 2, 0], np.uint8), read_round=np.array([0, 64, 0, 0], np.uint8),
               weak=np.array([[0, 1], [2 ** 31 - 1, 0], [0, 0], [3, 4]], np.int32), kept=np.array([[1, 2], [0, 0], [0, 0], [0, 2 ** 31 - 1]], np.int32))


@pytest.mark.parametrize("threads", [1, 7])
def test_a_literal_table(tmp_path, threads):
    hostio.set_threads(threads)
    names, lens = [f"r{i}/x extra" for i in range(4)], [1000, 300, 77, 400]
    write_fasta(tmp_path / "reads.fa", names, lens)
    r = hostio.Reads(str(tmp_path / "reads.fa"))
    try:
        hostio.write_graph_clean(str(tmp_path / "a.clean.tsv"), r, LITERAL)
    finally:
        r.close()
        hostio.set_threads(0)
    assert (tmp_path / "a.clean.tsv").read_text() == ("r0/x\t1000\tkept\t0\t0\t1\t1\t2\n" f"r1/x\t300\ttip\t64\t{2 ** 31 - 1}\t0\t0\t0\n"
                                                      "r2/x\t77\tflagged\t0\t0\t0\t0\t0\n" f"r3/x\t400\tkept\t0\t3\t0\t4\t{2 ** 31 - 1}\n")


def table(rng, n):
    state = rng.integers(0, 3, n).astype(np.uint8)
    return dict(read_state=state, read_round=np.where(state == 1, rng.integers(1, 65, n), 0).astype(np.uint8),
                weak=rng.integers(0, 50, (n, 2)).astype(np.int32), kept=rng.integers(0, 5, 2 * n).astype(np.int32))


def test_the_bytes_do_not_depend_on_the_thread_count(tmp_path, reads):
    res = table(np.random.default_rng(3), N_READS)
    want = clean_text([n.split()[0] for n in NAMES], LENGTHS, res)
    for threads in (1, 2, 7, 0):
        hostio.set_threads(threads)
        path = tmp_path / f"t{threads}.clean.tsv"
        hostio.write_graph_clean(str(path), reads, res)
        assert path.read_text() == want, threads
    assert want.count("\n") == N_READS and {ln.split("\t")[2] for ln in want.splitlines()} == set(STATES)


def test_no_reads(tmp_path):
    write_fasta(tmp_path / "none.fa", [], [])
    r = hostio.Reads(str(tmp_path / "none.fa"))
    try:
        hostio.write_graph_clean(str(tmp_path / "none.clean.tsv"), r, dict(read_state=[], read_round=[], weak=[], kept=[]))
    finally:
        r.close()
    assert (tmp_path / "none.clean.tsv").read_bytes() == b""


def test_what_is_refused(tmp_path, reads):
    good = table(np.random.default_rng(4), N_READS)
    for key, at, value in (("read_state", 3, 3), ("read_state", 0, 255), ("weak", 5, -1), ("kept", 2 * N_READS - 1, -7)):
        bad = {k: np.array(v).reshape(-1).copy() for k, v in good.items()}
        bad[key][at] = value
        with pytest.raises(hostio.HostError) as err:
            hostio.write_graph_clean(str(tmp_path / "bad.clean.tsv"), reads, bad)
        assert err.value.code == hostio.ERR_ARG and not (tmp_path / "bad.clean.tsv").exists(), (key, at)
    for key, size in (("read_state", N_READS - 1), ("read_round", N_READS + 1), ("weak", N_READS), ("kept", 2 * N_READS + 2)):
        with pytest.raises(ValueError, match="write_graph_clean: read_state and read_round"):
            hostio.write_graph_clean(str(tmp_path / "bad.clean.tsv"), reads, dict(good, **{key: np.zeros(size, good[key].dtype)}))
    with pytest.raises(hostio.HostError):
        hostio.write_graph_clean(str(tmp_path / "no" / "such" / "dir.clean.tsv"), reads, good)
    assert list(tmp_path.iterdir()) == []
