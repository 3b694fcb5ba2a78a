"""CPU: raft_host_write_components (include/raft_host_cc.h) -- the bytes of PREFIX.components.tsv and PREFIX.components.summary.tsv on a
literal table, stated by hand, with 1 and 7 workers; a larger table against a Python format; no reads; a table that names a component
or a first read outside the set, or an unwritable path, is refused."""
import numpy as np
import pytest
from raft_testlib import write_fasta
from test_host_paf_quality import N_READS, NAMES

from raft_amd import hostio

LENGTHS = [50 + i for i in range(N_READS)]


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    d = tmp_path_factory.mktemp("cc_reads")
    write_fasta(d / "reads.fa", NAMES, LENGTHS)
    r = hostio.Reads(str(d / "reads.fa"))
    yield r
    r.close()
    hostio.set_threads(0)


def table(component, degree, lens):
    """The rows of the components from the per-read arrays, as include/raft_hip_cc.h has them"""
    component, degree, lens = np.asarray(component, np.int32), np.asarray(degree, np.int32), np.asarray(lens, np.int64)
    C = int(component.max()) + 1 if component.size else 0
    first = np.array([np.flatnonzero(component == k)[0] for k in range(C)], np.int32)
    return dict(component=component, degree=degree, comp_first=first, comp_reads=np.bincount(component, minlength=C).astype(np.int32),
                comp_bases=np.bincount(component, weights=lens, minlength=C).astype(np.int64),
                comp_sides=np.bincount(component, weights=degree, minlength=C).astype(np.int64))


@pytest.mark.parametrize("threads", [1, 7])
def test_a_literal_table(tmp_path, threads):
    """Seven reads: {0, 3, 5}, {1, 6}, {2}, {4}"""
    hostio.set_threads(threads)
    names, lens = [f"r{i}/x extra" for i in range(7)], [1000, 2000, 300, 4000, 77, 6000, 7000]
    write_fasta(tmp_path / "reads.fa", names, lens)
    res = table([0, 1, 2, 0, 3, 0, 1], [2, 1, 0, 3, 0, 1, 1], lens)
    res["comp_sides"][1] = 2 ** 62 + 5                                 # (the writer prints what it is given)
    r = hostio.Reads(str(tmp_path / "reads.fa"))
    try:
        hostio.write_components(str(tmp_path / "x"), r, res)
    finally:
        r.close()
        hostio.set_threads(0)
    assert (tmp_path / "x.components.tsv").read_text() == ("r0/x\t1000\t0\t2\n" "r1/x\t2000\t1\t1\n" "r2/x\t300\t2\t0\n" "r3/x\t4000\t0\t3\n"
                                                           "r4/x\t77\t3\t0\n" "r5/x\t6000\t0\t1\n" "r6/x\t7000\t1\t1\n")
    assert (tmp_path / "x.components.summary.tsv").read_text() == ("0\t3\t11000\t6\tr0/x\n" f"1\t2\t9000\t{2 ** 62 + 5}\tr1/x\n"
                                                                   "2\t1\t300\t0\tr2/x\n" "3\t1\t77\t0\tr4/x\n")
    assert sorted(p.name for p in tmp_path.iterdir()) == ["reads.fa", "x.components.summary.tsv", "x.components.tsv"]


@pytest.mark.parametrize("threads", [1, 7])
def test_the_writer_equals_a_python_format(tmp_path, reads, threads):
    hostio.set_threads(threads)
    rng = np.random.default_rng(12)
    label = rng.integers(0, N_READS // 3, N_READS)
    _, first_seen, dense = np.unique(label, return_index=True, return_inverse=True)
    component = np.argsort(np.argsort(first_seen))[dense]              # dense ids in the order of the smallest members
    res = table(component, rng.integers(0, 2 ** 31 - 1, N_READS), LENGTHS)
    hostio.write_components(str(tmp_path / "y"), reads, res)
    per_read = "".join(f"{NAMES[i]}\t{LENGTHS[i]}\t{res['component'][i]}\t{res['degree'][i]}\n" for i in range(N_READS))
    per_comp = "".join(f"{k}\t{res['comp_reads'][k]}\t{res['comp_bases'][k]}\t{res['comp_sides'][k]}\t{NAMES[res['comp_first'][k]]}\n"
                       for k in range(res["comp_first"].size))
    assert (tmp_path / "y.components.tsv").read_bytes() == per_read.encode()
    assert (tmp_path / "y.components.summary.tsv").read_bytes() == per_comp.encode()
    assert np.all(np.diff(res["comp_first"]) > 0) and res["comp_reads"].sum() == N_READS


def test_no_reads(tmp_path):
    (tmp_path / "empty.fa").write_text("")
    r = hostio.Reads(str(tmp_path / "empty.fa"))
    try:
        assert r.n == 0
        hostio.write_components(str(tmp_path / "e"), r, table([], [], []))
        assert (tmp_path / "e.components.tsv").read_bytes() == b"" and (tmp_path / "e.components.summary.tsv").read_bytes() == b""
    finally:
        r.close()


def test_the_refusals(tmp_path, reads):
    sound = table(np.arange(N_READS) // 2, np.ones(N_READS), LENGTHS)
    for key in ("component", "degree", "comp_reads", "comp_bases", "comp_sides"):
        w = dict(sound)
        w[key] = w[key][:-1]
        with pytest.raises(ValueError):
            hostio.write_components(str(tmp_path / "y"), reads, w)
    for key, bad in (("component", sound["comp_first"].size), ("component", -1), ("comp_first", N_READS), ("comp_first", -1), ("comp_first", 2 ** 31 - 1)):
        w = {k: v.copy() for k, v in sound.items()}
        w[key][3] = bad
        with pytest.raises(hostio.HostError):
            hostio.write_components(str(tmp_path / "y"), reads, w)
    assert not (tmp_path / "y.components.tsv").exists() and not (tmp_path / "y.components.summary.tsv").exists()
    with pytest.raises(hostio.HostError):
        hostio.write_components(str(tmp_path / "no" / "such" / "dir"), reads, sound)
    hostio.write_components(str(tmp_path / "y"), reads, sound)
    assert (tmp_path / "y.components.tsv").exists() and (tmp_path / "y.components.summary.tsv").exists()
