"""CPU: raft_host_write_string_graph (include/raft_host_sg.h) -- the bytes of PREFIX.string_graph.gfa and PREFIX.string_graph.tsv on a
literal table, stated by hand, with 1 and 7 workers; a larger table against a writer in Python (``gfa_text``, ``tsv_text``: the CLI's
GPU test compares with the same two); no reads; a list that names a node outside the set or an end of a flagged read, or an
unwritable path, is refused before anything is written."""
import numpy as np
import pytest
from raft_testlib import write_fasta
from test_host_paf_quality import N_READS, NAMES

from raft_amd import hostio

LENGTHS = [50 + i for i in range(N_READS)]
SKIPPED = 16


def gfa_text(names, lengths, res):
    """The GFA as include/raft_host_sg.h states it, from the result of ``Engine.string_graph`` (or the oracle's)"""
    out = ["H\tVN:Z:1.0\n"]
    out += [f"S\t{names[r]}\t*\tLN:i:{lengths[r]}\n" for r in range(len(names)) if not res["flags"][r] & SKIPPED]
    for u, w, span in zip(res["edge_u"].tolist(), res["edge_w"].tolist(), res["edge_span"].tolist()):
        out.append(f"L\t{names[u >> 1]}\t{'+' if u & 1 else '-'}\t{names[w >> 1]}\t{'-' if w & 1 else '+'}\t{span}M\n")
    return "".join(out)


def tsv_text(names, lengths, res):
    arcs, kept = np.asarray(res["arcs"]).reshape(-1, 2), np.asarray(res["kept"]).reshape(-1, 2)
    return "".join(f"{names[r]}\t{lengths[r]}\t{arcs[r, 0]}\t{kept[r, 0]}\t{arcs[r, 1]}\t{kept[r, 1]}\n" for r in range(len(names)))


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    d = tmp_path_factory.mktemp("sg_reads")
    write_fasta(d / "reads.fa", NAMES, LENGTHS)
    r = hostio.Reads(str(d / "reads.fa"))
    yield r
    r.close()
    hostio.set_threads(0)


def table(n, flagged, edges, rng=None):
    rng = rng or np.random.default_rng(0)
    flags = np.zeros(n, np.uint8)
    flags[list(flagged)] = SKIPPED
    flags |= rng.integers(0, 16, n).astype(np.uint8)                   # (the other bits have no say)
    e = np.array(edges, np.int64).reshape(-1, 3)
    return dict(arcs=rng.integers(0, 2 ** 31 - 1, (n, 2)).astype(np.int32), kept=rng.integers(0, 9, (n, 2)).astype(np.int32), flags=flags,
                edge_u=e[:, 0].astype(np.int32), edge_w=e[:, 1].astype(np.int32), edge_span=e[:, 2].astype(np.int32))


@pytest.mark.parametrize("threads", [1, 7])
def test_a_literal_table(tmp_path, threads):
    """Five reads, read 2 flagged: 0 -> 1 on '+', 1's 3' end against 3's 3' end, 4's 5' end against 0's 5' end"""
    hostio.set_threads(threads)
    names, lens = [f"r{i}/x extra" for i in range(5)], [1000, 2000, 300, 4000, 77]
    write_fasta(tmp_path / "reads.fa", names, lens)
    res = table(5, [2], [(1, 2, 640), (3, 7, 1999), (8, 0, 2147483647)])
    res["flags"][:] = [0, 15, 16, 3, 8]
    res["arcs"][:] = [[0, 1], [1, 2], [0, 0], [0, 1], [1, 0]]
    res["kept"][:] = [[0, 1], [1, 1], [0, 0], [0, 1], [1, 0]]
    r = hostio.Reads(str(tmp_path / "reads.fa"))
    try:
        hostio.write_string_graph(str(tmp_path / "x"), r, res)
    finally:
        r.close()
        hostio.set_threads(0)
    assert (tmp_path / "x.string_graph.gfa").read_text() == ("H\tVN:Z:1.0\n" "S\tr0/x\t*\tLN:i:1000\n" "S\tr1/x\t*\tLN:i:2000\n" "S\tr3/x\t*\tLN:i:4000\n"
                                                             "S\tr4/x\t*\tLN:i:77\n" "L\tr0/x\t+\tr1/x\t+\t640M\n" "L\tr1/x\t+\tr3/x\t-\t1999M\n"
                                                             "L\tr4/x\t-\tr0/x\t+\t2147483647M\n")
    assert (tmp_path / "x.string_graph.tsv").read_text() == ("r0/x\t1000\t0\t0\t1\t1\n" "r1/x\t2000\t1\t1\t2\t1\n" "r2/x\t300\t0\t0\t0\t0\n"
                                                             "r3/x\t4000\t0\t0\t1\t1\n" "r4/x\t77\t1\t1\t0\t0\n")
    assert sorted(p.name for p in tmp_path.iterdir()) == ["reads.fa", "x.string_graph.gfa", "x.string_graph.tsv"]
    short = [n.split()[0] for n in names]
    assert gfa_text(short, lens, res) == (tmp_path / "x.string_graph.gfa").read_text() and tsv_text(short, lens, res) == (tmp_path / "x.string_graph.tsv").read_text()


def big_table(rng):
    flagged = set(rng.choice(N_READS, N_READS // 5, replace=False).tolist())
    free = np.array([r for r in range(N_READS) if r not in flagged])
    m = 3 * N_READS + 7
    u = 2 * rng.choice(free, m) + rng.integers(0, 2, m)
    w = 2 * rng.choice(free, m) + rng.integers(0, 2, m)
    return table(N_READS, flagged, np.stack([u, w, rng.integers(1, 2 ** 31 - 1, m)], axis=1), rng)


def test_the_writer_equals_a_python_format_and_one_thread_equals_many(tmp_path, reads):
    res = big_table(np.random.default_rng(12))
    got = {}
    for threads in (1, 2, 7, 0):
        hostio.set_threads(threads)
        hostio.write_string_graph(str(tmp_path / f"y{threads}"), reads, res)
        got[threads] = ((tmp_path / f"y{threads}.string_graph.gfa").read_bytes(), (tmp_path / f"y{threads}.string_graph.tsv").read_bytes())
    assert got[1] == (gfa_text(NAMES, LENGTHS, res).encode(), tsv_text(NAMES, LENGTHS, res).encode())
    assert got[2] == got[1] and got[7] == got[1] and got[0] == got[1]
    assert got[1][0].count(b"\nS\t") == N_READS - N_READS // 5 and got[1][0].count(b"\nL\t") == 3 * N_READS + 7
    # the arrays as the engine returns them ([n_reads, 2]) or flat
    flat = dict(res, arcs=res["arcs"].ravel(), kept=res["kept"].ravel())
    hostio.write_string_graph(str(tmp_path / "flat"), reads, flat)
    assert (tmp_path / "flat.string_graph.tsv").read_bytes() == got[1][1]


def test_no_reads_and_no_edges(tmp_path, reads):
    (tmp_path / "empty.fa").write_text("")
    r = hostio.Reads(str(tmp_path / "empty.fa"))
    try:
        assert r.n == 0
        hostio.write_string_graph(str(tmp_path / "e"), r, table(0, [], []))
        assert (tmp_path / "e.string_graph.gfa").read_bytes() == b"H\tVN:Z:1.0\n" and (tmp_path / "e.string_graph.tsv").read_bytes() == b""
    finally:
        r.close()
    res = table(N_READS, range(N_READS), [])
    hostio.write_string_graph(str(tmp_path / "all"), reads, res)
    assert (tmp_path / "all.string_graph.gfa").read_bytes() == b"H\tVN:Z:1.0\n"
    assert (tmp_path / "all.string_graph.tsv").read_bytes() == tsv_text(NAMES, LENGTHS, res).encode()


def test_the_refusals(tmp_path, reads):
    sound = big_table(np.random.default_rng(3))
    for key in ("arcs", "kept", "flags", "edge_w", "edge_span"):
        w = dict(sound)
        w[key] = w[key][:-1]
        with pytest.raises(ValueError):
            hostio.write_string_graph(str(tmp_path / "y"), reads, w)
    flagged = int(np.flatnonzero(sound["flags"] & SKIPPED)[0])
    for key, bad in (("edge_u", 2 * N_READS), ("edge_u", -1), ("edge_w", 2 * N_READS), ("edge_w", -1), ("edge_w", 2 ** 31 - 1), ("edge_u", -2 ** 31),
                     ("edge_u", 2 * flagged), ("edge_w", 2 * flagged + 1)):
        w = {k: v.copy() for k, v in sound.items()}
        w[key][-1 if bad < 0 else 3] = bad
        with pytest.raises(hostio.HostError):
            hostio.write_string_graph(str(tmp_path / "y"), reads, w)
    assert not (tmp_path / "y.string_graph.gfa").exists() and not (tmp_path / "y.string_graph.tsv").exists()
    with pytest.raises(hostio.HostError):
        hostio.write_string_graph(str(tmp_path / "no" / "such" / "dir"), reads, sound)
    hostio.write_string_graph(str(tmp_path / "y"), reads, sound)
    assert (tmp_path / "y.string_graph.gfa").exists() and (tmp_path / "y.string_graph.tsv").exists()
