"""CPU: raft_host_write_containment and raft_host_write_unitig_depth (include/raft_host_ctn.h) -- the bytes of PREFIX.containment.tsv and
PREFIX.unitigs.depth.tsv on a literal table, stated by hand, with 1 and 7 workers, with and without the placed columns; a larger table
against a Python format; no reads; a table that names a parent, a root or a unitig outside its range, or an unwritable path, is refused."""
import numpy as np
import pytest
from ctn_testlib import HAS_PARENT, PARENT_REV, PER_READ, ROOT_REV, UNPLACED_VIEW
from raft_testlib import write_fasta
from test_host_paf_quality import N_READS, NAMES

from raft_amd import hostio

LENGTHS = [50 + i for i in range(N_READS)]


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    d = tmp_path_factory.mktemp("ctn_reads")
    write_fasta(d / "reads.fa", NAMES, LENGTHS)
    r = hostio.Reads(str(d / "reads.fa"))
    yield r
    r.close()
    hostio.set_threads(0)


def containment_text(names, lens, res, placed=None):
    """PREFIX.containment.tsv as include/raft_host_ctn.h has it"""
    out = []
    for i, name in enumerate(names):
        f = int(res["flags"][i])
        row = [name, lens[i]]
        row += [names[res["parent"][i]], "-" if f & PARENT_REV else "+", res["pos"][i], res["span"][i]] if res["parent"][i] >= 0 else ["*", "*", 0, 0]
        row += [names[res["root"][i]], "-" if f & ROOT_REV else "+", res["root_pos"][i], res["depth"][i], res["children"][i], res["tree_reads"][i], res["tree_bases"][i]]
        if placed is not None and placed["placed_unitig"][i] >= 0:
            row += [placed["placed_unitig"][i], placed["start"][i], "-" if placed["placed_orient"][i] else "+"]
        else:
            row += ["*", 0, "*"]
        out.append("\t".join(str(x) for x in row) + "\n")
    return "".join(out)


def depth_text(utg_reads, utg_length, placed):
    return "".join(f"{u}\t{utg_reads[u]}\t{utg_length[u]}\t{placed['placed_reads'][u]}\t{placed['placed_bases'][u]}\t{placed['depth_permille'][u]}\n"
                   for u in range(len(utg_reads)))


def forest(rows):
    """rows of the eleven per-read values in the order of ctn_testlib.PER_READ"""
    a = np.asarray(rows, np.int64).reshape(-1, len(PER_READ))
    return {k: np.ascontiguousarray(a[:, j]).astype(dt) for j, (k, dt) in enumerate(PER_READ.items())}


LITERAL = forest([[-1, 0, 0, 0, 0, 0, 2, 0, 3, 2 ** 40 + 7, 2],                                    # r0: a root with a tree
                  [0, 10, 300, 0, 10, 1, 1, HAS_PARENT, 0, 0, 0],                                  # r1 in r0, '+'
                  [1, 5, 77, 0, 218, 2, 0, HAS_PARENT | PARENT_REV | ROOT_REV, 0, 0, 0],           # r2 in r1, '-'
                  [0, 600, 400, 0, 600, 1, 0, HAS_PARENT | PARENT_REV | ROOT_REV | UNPLACED_VIEW, 0, 0, 0],
                  [-1, 0, 0, 4, 0, 0, 0, UNPLACED_VIEW | 16, 0, 0, 0]])                            # r4: an orphan
PLACED = dict(placed_unitig=np.array([0, 0, 0, 0, -1], np.int32), start=np.array([2 ** 33, 2 ** 33 + 10, 2 ** 33 + 218, 2 ** 33 + 600, 0], np.int64),
              placed_orient=np.array([0, 0, 1, 1, 0], np.uint8), placed_reads=np.array([4], np.int32), placed_bases=np.array([1777], np.int64),
              depth_permille=np.array([1777], np.int64))


@pytest.mark.parametrize("threads", [1, 7])
def test_a_literal_table(tmp_path, threads):
    hostio.set_threads(threads)
    names, lens = [f"r{i}/x extra" for i in range(5)], [1000, 300, 77, 400, 90]
    write_fasta(tmp_path / "reads.fa", names, lens)
    r = hostio.Reads(str(tmp_path / "reads.fa"))
    try:
        hostio.write_containment(str(tmp_path / "a.containment.tsv"), r, LITERAL)
        hostio.write_containment(str(tmp_path / "b.containment.tsv"), r, LITERAL, PLACED)
        hostio.write_unitig_depth(str(tmp_path / "b.unitigs.depth.tsv"), [1], [1000], PLACED)
    finally:
        r.close()
        hostio.set_threads(0)
    head = [f"r0/x\t1000\t*\t*\t0\t0\tr0/x\t+\t0\t0\t2\t3\t{2 ** 40 + 7}", "r1/x\t300\tr0/x\t+\t10\t300\tr0/x\t+\t10\t1\t1\t0\t0",
            "r2/x\t77\tr1/x\t-\t5\t77\tr0/x\t-\t218\t2\t0\t0\t0", "r3/x\t400\tr0/x\t-\t600\t400\tr0/x\t-\t600\t1\t0\t0\t0", "r4/x\t90\t*\t*\t0\t0\tr4/x\t+\t0\t0\t0\t0\t0"]
    assert (tmp_path / "a.containment.tsv").read_text() == "".join(h + "\t*\t0\t*\n" for h in head)
    tail = [f"0\t{2 ** 33}\t+", f"0\t{2 ** 33 + 10}\t+", f"0\t{2 ** 33 + 218}\t-", f"0\t{2 ** 33 + 600}\t-", "*\t0\t*"]
    assert (tmp_path / "b.containment.tsv").read_text() == "".join(h + "\t" + t + "\n" for h, t in zip(head, tail))
    assert (tmp_path / "b.unitigs.depth.tsv").read_text() == "0\t1\t1000\t4\t1777\t1777\n"
    short = [n.split()[0] for n in names]
    assert containment_text(short, lens, LITERAL) == (tmp_path / "a.containment.tsv").read_text()
    assert containment_text(short, lens, LITERAL, PLACED) == (tmp_path / "b.containment.tsv").read_text()


@pytest.mark.parametrize("threads", [1, 7])
def test_the_writers_equal_a_python_format(tmp_path, reads, threads):
    hostio.set_threads(threads)
    rng = np.random.default_rng(21)
    n = N_READS
    res = {k: rng.integers(0, 2 ** 31 - 1 if dt != np.uint8 else 32, n).astype(dt) for k, dt in PER_READ.items()}
    res["parent"] = rng.integers(-1, n, n).astype(np.int32)
    res["root"] = rng.integers(0, n, n).astype(np.int32)
    res["tree_bases"] = rng.integers(0, 2 ** 62, n)
    U = 40
    placed = dict(placed_unitig=rng.integers(-1, U, n).astype(np.int32), start=rng.integers(-5, 2 ** 40, n), placed_orient=rng.integers(0, 2, n).astype(np.uint8),
                  placed_reads=rng.integers(0, 2 ** 31 - 1, U).astype(np.int32), placed_bases=rng.integers(0, 2 ** 62, U), depth_permille=rng.integers(0, 2 ** 62, U))
    utg_reads, utg_length = rng.integers(1, 100, U).astype(np.int32), rng.integers(0, 2 ** 40, U)
    hostio.write_containment(str(tmp_path / "y.tsv"), reads, res, placed)
    hostio.write_containment(str(tmp_path / "z.tsv"), reads, res)
    hostio.write_unitig_depth(str(tmp_path / "d.tsv"), utg_reads, utg_length, placed)
    assert (tmp_path / "y.tsv").read_bytes() == containment_text(NAMES, LENGTHS, res, placed).encode()
    assert (tmp_path / "z.tsv").read_bytes() == containment_text(NAMES, LENGTHS, res).encode()
    assert (tmp_path / "d.tsv").read_bytes() == depth_text(utg_reads, utg_length, placed).encode()


def test_no_reads_and_no_unitigs(tmp_path):
    (tmp_path / "empty.fa").write_text("")
    r = hostio.Reads(str(tmp_path / "empty.fa"))
    try:
        assert r.n == 0
        hostio.write_containment(str(tmp_path / "e.tsv"), r, forest([]))
        none = dict(placed_reads=[], placed_bases=[], depth_permille=[])
        hostio.write_unitig_depth(str(tmp_path / "d.tsv"), [], [], none)
        assert (tmp_path / "e.tsv").read_bytes() == b"" and (tmp_path / "d.tsv").read_bytes() == b""
    finally:
        r.close()


def test_the_refusals(tmp_path, reads):
    n = N_READS
    sound = forest([[-1, 0, 0, i, 0, 0, 0, 0, 0, 0, 0] for i in range(n)])
    placed = dict(placed_unitig=np.zeros(n, np.int32), start=np.zeros(n, np.int64), placed_orient=np.zeros(n, np.uint8))
    for key in [k for k in PER_READ if k != "tree_depth"]:             # (the file has no column for it)
        w = dict(sound)
        w[key] = w[key][:-1]
        with pytest.raises(ValueError):
            hostio.write_containment(str(tmp_path / "y.tsv"), reads, w)
    for key in placed:
        w = dict(placed)
        w[key] = w[key][:-1]
        with pytest.raises(ValueError):
            hostio.write_containment(str(tmp_path / "y.tsv"), reads, sound, w)
    for key, bad in (("parent", n), ("parent", -2), ("root", n), ("root", -1), ("root", 2 ** 31 - 1)):
        w = {k: v.copy() for k, v in sound.items()}
        w[key][3] = bad
        with pytest.raises(hostio.HostError):
            hostio.write_containment(str(tmp_path / "y.tsv"), reads, w)
    w = {k: v.copy() for k, v in placed.items()}
    w["placed_unitig"][5] = -2
    with pytest.raises(hostio.HostError):
        hostio.write_containment(str(tmp_path / "y.tsv"), reads, sound, w)
    assert not (tmp_path / "y.tsv").exists()
    with pytest.raises(hostio.HostError):
        hostio.write_containment(str(tmp_path / "no" / "such" / "dir.tsv"), reads, sound)
    with pytest.raises(hostio.HostError):
        hostio.write_unitig_depth(str(tmp_path / "no" / "such" / "dir.tsv"), [1], [5], dict(placed_reads=[1], placed_bases=[5], depth_permille=[1000]))
    with pytest.raises(ValueError):
        hostio.write_unitig_depth(str(tmp_path / "d.tsv"), [1, 2], [5], dict(placed_reads=[1], placed_bases=[5], depth_permille=[1000]))
    hostio.write_containment(str(tmp_path / "y.tsv"), reads, sound, placed)
    assert (tmp_path / "y.tsv").exists()
