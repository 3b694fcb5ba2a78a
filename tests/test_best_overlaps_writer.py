"""CPU: raft_host_write_best_overlaps (include/raft_host_best.h) -- the bytes of PREFIX.best_overlaps.tsv equal a Python format: no
reads, reads without any best overlap, both strands, mutual and not, skipped reads; a partner that is no read and an unwritable
path are refused."""
import numpy as np
import pytest
from raft_testlib import write_fasta
from test_host_paf_quality import N_READS, NAMES

from raft_amd import hostio


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    d = tmp_path_factory.mktemp("best_reads")
    write_fasta(d / "reads.fa", NAMES, [50 + i for i in range(N_READS)])
    r = hostio.Reads(str(d / "reads.fa"))
    yield r
    r.close()
    hostio.set_threads(0)


def want_text(names, lengths, partner, span, flags):
    lines = []
    for r, name in enumerate(names):
        f = [name, str(int(lengths[r]))]
        for e in range(2):
            p, bits = int(partner[r, e]), int(flags[r]) >> (2 * e)
            f += ["*", "*", "0", "0"] if p < 0 else [names[p], "-" if bits & 1 else "+", str(int(span[r, e])), "1" if bits & 2 else "0"]
        lines.append("\t".join(f + ["1" if flags[r] & 16 else "0"]) + "\n")
    return "".join(lines).encode()


@pytest.mark.parametrize("threads", [1, 7])
def test_the_writer_equals_a_python_format(tmp_path, reads, threads):
    hostio.set_threads(threads)
    rng = np.random.default_rng(12)
    partner = rng.integers(0, N_READS, (N_READS, 2)).astype(np.int32)
    span = rng.integers(1, 2 ** 31, (N_READS, 2), dtype=np.int64).astype(np.int32)
    flags = rng.integers(0, 16, N_READS).astype(np.uint8)             # (every combination of the two strands and the two mutual bits)
    partner[rng.random((N_READS, 2)) < 0.3] = -1
    partner[0], partner[1, 0], partner[2, 1] = -1, N_READS - 1, 0
    span[1, 0] = 2 ** 31 - 1
    flags[3], partner[3] = 16, -1                                      # a skipped read: no best overlap at either end
    flags[4] |= 16                                                     # (the writer prints what it is given)
    hostio.write_best_overlaps(str(tmp_path / "x.best_overlaps.tsv"), reads, partner, span, flags)
    got = (tmp_path / "x.best_overlaps.tsv").read_bytes()
    assert got == want_text(NAMES, [50 + r for r in range(N_READS)], partner, span, flags)
    lines = got.decode().split("\n")
    assert lines[0] == f"{NAMES[0]}\t50\t*\t*\t0\t0\t*\t*\t0\t0\t{int(flags[0]) >> 4}" and lines[3].endswith("\t*\t*\t0\t0\t*\t*\t0\t0\t1")
    assert all(len(l.split("\t")) == 11 for l in lines[:-1]) and lines[-1] == "" and len(lines) == N_READS + 1
    assert any("\t+\t" in l for l in lines) and any("\t-\t" in l for l in lines)


def test_reads_without_any_best_overlap(tmp_path, reads):
    partner, span, flags = np.full((N_READS, 2), -1, np.int32), np.zeros((N_READS, 2), np.int32), np.zeros(N_READS, np.uint8)
    hostio.write_best_overlaps(str(tmp_path / "none.tsv"), reads, partner, span, flags)
    assert (tmp_path / "none.tsv").read_bytes() == "".join(f"{NAMES[r]}\t{50 + r}\t*\t*\t0\t0\t*\t*\t0\t0\t0\n" for r in range(N_READS)).encode()


def test_no_reads(tmp_path):
    (tmp_path / "empty.fa").write_text("")
    r = hostio.Reads(str(tmp_path / "empty.fa"))
    try:
        assert r.n == 0
        hostio.write_best_overlaps(str(tmp_path / "e.tsv"), r, np.zeros((0, 2), np.int32), np.zeros((0, 2), np.int32), np.zeros(0, np.uint8))
        assert (tmp_path / "e.tsv").read_bytes() == b""
    finally:
        r.close()


def test_the_refusals(tmp_path, reads):
    partner, span, flags = np.full((N_READS, 2), -1, np.int32), np.zeros((N_READS, 2), np.int32), np.zeros(N_READS, np.uint8)
    with pytest.raises(ValueError):
        hostio.write_best_overlaps(str(tmp_path / "y.tsv"), reads, partner[:-1], span, flags)
    with pytest.raises(ValueError):
        hostio.write_best_overlaps(str(tmp_path / "y.tsv"), reads, partner, span, flags[:-1])
    for bad in (N_READS, -2, 2 ** 31 - 1):
        p = partner.copy()
        p[N_READS // 2, 1] = bad
        with pytest.raises(hostio.HostError):
            hostio.write_best_overlaps(str(tmp_path / "y.tsv"), reads, p, span, flags)
    assert not (tmp_path / "y.tsv").exists()
    with pytest.raises(hostio.HostError):
        hostio.write_best_overlaps(str(tmp_path / "no" / "such" / "dir.tsv"), reads, partner, span, flags)
