"""CPU: raft_host_paf_parse_with / raft_host_paf_load_with (include/raft_host_end.h) -- the tokeniser under a mask of columns -- and
raft_host_write_overlap_ends.  Under columns = 0, 1, 2, 3 the six columns and the symmetric flag are the plain parser's, the quality
columns those of raft_host_paf_parse_quality, and the strand byte equals a ``split("\\t")`` restatement of the text: field 5 of '+',
'-', '-x', '*' and nothing at all, lines of ten to fifteen fields, CRLF, a last line without a newline, a .gz copy; 0 lines, 1 line,
and enough lines for the tokeniser's chunks, with 1 and 7 worker threads.  The writer's bytes equal a Python format."""
import ctypes as C
import gzip

import numpy as np
import pytest
from raft_testlib import write_fasta
from test_host_paf_quality import N_READS, NAMES, c_num, digits

from raft_amd import hostio

STRANDS = ["+", "-", "-x", "*", "", "+-", "--"]


def restate(text: str):
    """-> the strand byte and the six columns of every line with ten fields or more."""
    index = {n: i for i, n in enumerate(NAMES)}
    rows = []
    for line in text.split("\n"):
        if len(line) > 1 and line.endswith("\r"):
            line = line[:-1]
        f = line.split("\t")
        if len(f) < 10:
            continue
        rows.append((index[f[0]], c_num(f[2]), c_num(f[3]), index[f[5]], c_num(f[7]), c_num(f[8]), 1 if f[4][:1] == "-" else 0))
    return [np.array([r[k] for r in rows], np.uint8 if k == 6 else np.int32) for k in range(7)]


def make_text(n_lines: int, seed: int, eol: str = "\n", mirror_first: bool = False, last_newline: bool = True) -> str:
    rng = np.random.default_rng(seed)
    tail = ["60", "tp:A:P", "cm:i:100", "s1:i:90", "dv:f:0.01", "rl:i:0"]
    lines = []
    for i in range(n_lines):
        n_fields = (11, 12, 15, 10, 9, 12)[i % 6] if i else 12
        a, b = int(rng.integers(0, N_READS)), int(rng.integers(0, N_READS))
        coord = [digits(rng, int(rng.integers(1, 8))) for _ in range(4)]
        f = [NAMES[a], "20000", coord[0], coord[1], STRANDS[(i + i // 7) % len(STRANDS)], NAMES[b], "25000", coord[2], coord[3],
             digits(rng, 1 + i % 6), digits(rng, 1 + i % 5)] + tail
        lines.append("\t".join(f[:n_fields]))
    if mirror_first and lines:
        f = lines[0].split("\t")
        lines.insert(n_lines // 2, "\t".join([f[5], f[6], f[7], f[8], f[4], f[0], f[1], f[2], f[3]] + f[9:11]))
    return eol.join(lines) + (eol if last_newline and lines else "")


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    d = tmp_path_factory.mktemp("strand_reads")
    write_fasta(d / "reads.fa", NAMES, [50 + i for i in range(N_READS)])
    r = hostio.Reads(str(d / "reads.fa"))
    yield r
    r.close()
    hostio.set_threads(0)


def load_with(path, reads, columns: int, two_steps: bool):
    """The object raft_host_paf_load_with / _parse_with makes under ``columns`` -> six columns, the quality columns or None, the strand or None, the flag."""
    lib = hostio.load_library()
    h, err = C.c_void_p(), C.create_string_buffer(256)
    if two_steps:
        t = C.c_void_p()
        assert lib.raft_host_text_read(str(path).encode(), C.byref(t)) == hostio.OK
        rc = lib.raft_host_paf_parse_with(t, reads._h, columns, C.byref(h), err, 256)
        lib.raft_host_text_free(t)
    else:
        rc = lib.raft_host_paf_load_with(str(path).encode(), reads._h, columns, C.byref(h), err, 256)
    assert rc == hostio.OK, (rc, err.value)
    n = lib.raft_host_paf_count(h)
    view = lambda p, dt: np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.empty(0, dt)
    cols = [view(lib.raft_host_paf_column(h, k), np.int32) for k in range(6)]
    quality = [view(lib.raft_host_paf_quality(h, k), np.int32) for k in range(2)] if lib.raft_host_paf_quality(h, 0) else None
    assert bool(lib.raft_host_paf_quality(h, 0)) == bool(lib.raft_host_paf_quality(h, 1))
    strand = view(lib.raft_host_paf_strand(h), np.uint8) if lib.raft_host_paf_strand(h) else None
    flag = int(lib.raft_host_paf_symmetric(h))
    lib.raft_host_paf_free(h)
    return cols, quality, strand, flag


def compare(path, text, reads, what):
    want = restate(text)
    plain, flag = hostio.load_paf(str(path), reads, with_flag=True)
    with_quality = hostio.load_paf(str(path), reads, quality=True)
    assert all(np.array_equal(a, b) for a, b in zip(plain, want[:6])), what
    for columns in (0, 1, 2, 3):
        for two_steps in (False, True):
            cols, quality, strand, got_flag = load_with(path, reads, columns, two_steps)
            ctx = (what, columns, two_steps)
            assert all(a.dtype == np.int32 and np.array_equal(a, b) for a, b in zip(cols, plain)) and got_flag == flag, ctx
            assert (quality is not None) == bool(columns & hostio.PAF_QUALITY) and (strand is not None) == bool(columns & hostio.PAF_STRAND), ctx
            if quality is not None:
                assert all(np.array_equal(a, b) for a, b in zip(quality, with_quality[6:])), ctx
            if strand is not None:
                assert strand.dtype == np.uint8 and np.array_equal(strand, want[6]), ctx
    # ... and through the Python binding: the strand is the last column, behind the quality columns where both are asked for
    for quality in (False, True):
        for two_steps in (False, True):
            got, got_flag = hostio.load_paf(str(path), reads, with_flag=True, two_steps=two_steps, quality=quality, strand=True)
            assert len(got) == (9 if quality else 7) and got_flag == flag and got[-1].dtype == np.uint8 and np.array_equal(got[-1], want[6])
            assert all(np.array_equal(a, b) for a, b in zip(got[:-1], with_quality if quality else plain))
    return want, flag


@pytest.mark.parametrize("threads", [1, 7])
@pytest.mark.parametrize("n_lines", [0, 1, 300, 30000], ids=["empty", "one line", "one chunk", "chunks"])
def test_the_strand_equals_a_python_split(tmp_path, reads, threads, n_lines):
    hostio.set_threads(threads)
    text = make_text(n_lines, seed=n_lines + 1)
    assert (len(text) > (1 << 20)) == (n_lines == 30000)              # host_io.cpp: a text below 1 MiB is one chunk
    if n_lines == 0:
        text = "\n"                                                    # (an empty file is refused before the tokeniser sees it)
    (tmp_path / "a.paf").write_text(text)
    want, flag = compare(tmp_path / "a.paf", text, reads, "plain")
    assert flag == 0 and want[0].size == n_lines - n_lines // 6          # every sixth line has nine fields
    if n_lines >= 300:
        fields = [ln.split("\t")[4] for ln in text.split("\n") if ln.count("\t") >= 9]
        assert set(fields) == set(STRANDS) and 0 < int(want[6].sum()) < want[6].size
        assert [int(x) for x in want[6][:7]] == [1 if s[:1] == "-" else 0 for s in fields[:7]]
        assert {ln.count("\t") + 1 for ln in text.split("\n") if ln.count("\t") >= 9} == {10, 11, 12, 15}
    with gzip.open(tmp_path / "a.paf.gz", "wt", newline="") as f:
        f.write(text)
    compare(tmp_path / "a.paf.gz", text, reads, "gz")
    crlf = make_text(n_lines, seed=n_lines + 1, eol="\r\n") or "\r\n"
    (tmp_path / "crlf.paf").write_bytes(crlf.encode())
    got, _ = compare(tmp_path / "crlf.paf", crlf, reads, "crlf")
    assert all(np.array_equal(a, b) for a, b in zip(got, want))          # the carriage return belongs to no field
    if n_lines:
        mirrored = make_text(n_lines, seed=n_lines + 1, mirror_first=True, last_newline=False)
        (tmp_path / "m.paf").write_text(mirrored)
        _, flag = compare(tmp_path / "m.paf", mirrored, reads, "mirror of the first record, no last newline")
        assert flag == 1


def test_a_mask_with_another_bit_is_refused(tmp_path, reads):
    lib = hostio.load_library()
    (tmp_path / "a.paf").write_text(make_text(20, seed=3))
    for columns in (4, 7, -1, 1 << 20):
        h = C.c_void_p(1)
        assert lib.raft_host_paf_load_with(str(tmp_path / "a.paf").encode(), reads._h, columns, C.byref(h), None, 0) == hostio.ERR_ARG and not h.value
        t = C.c_void_p()
        assert lib.raft_host_text_read(str(tmp_path / "a.paf").encode(), C.byref(t)) == hostio.OK
        h = C.c_void_p(1)
        assert lib.raft_host_paf_parse_with(t, reads._h, columns, C.byref(h), None, 0) == hostio.ERR_ARG and not h.value
        lib.raft_host_text_free(t)
    assert not lib.raft_host_paf_strand(None)


def test_an_unknown_name_is_the_plain_parsers_error(tmp_path, reads):
    text = make_text(20, seed=2) + "\t".join(["nobody", "1", "0", "1", "-", NAMES[0], "1", "0", "1", "0", "0"]) + "\n"
    (tmp_path / "a.paf").write_text(text)
    for quality in (False, True):
        with pytest.raises(hostio.HostError) as e:
            hostio.load_paf(str(tmp_path / "a.paf"), reads, quality=quality, strand=True)
        assert e.value.code == hostio.ERR_UNKNOWN_NAME and e.value.what == "nobody"


@pytest.mark.parametrize("threads", [1, 7])
def test_the_writer_equals_a_python_format(tmp_path, reads, threads):
    hostio.set_threads(threads)
    rng = np.random.default_rng(11)
    counts = rng.integers(0, 2 ** 31, (5, N_READS), dtype=np.int64).astype(np.int32)
    counts[:, 0] = 0
    counts[:, 1] = 2 ** 31 - 1
    status = rng.integers(0, 5, N_READS).astype(np.uint8)
    hostio.write_overlap_ends(str(tmp_path / "x.overlap_ends.tsv"), reads, counts, status)
    want = "".join("\t".join([NAMES[r], str(50 + r)] + [str(int(counts[k, r])) for k in range(5)] + [str(int(status[r]))]) + "\n" for r in range(N_READS))
    assert (tmp_path / "x.overlap_ends.tsv").read_bytes() == want.encode()
    with pytest.raises(ValueError):
        hostio.write_overlap_ends(str(tmp_path / "y.tsv"), reads, counts[:4], status)
    with pytest.raises(hostio.HostError):
        hostio.write_overlap_ends(str(tmp_path / "no" / "such" / "dir.tsv"), reads, counts, status)
