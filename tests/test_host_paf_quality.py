"""CPU: raft_host_paf_parse_quality / raft_host_paf_load_quality (include/raft_host_flt.h) -- the tokeniser that also keeps PAF
fields 10 and 11 -- against a ``split("\\t")`` restatement on generated text: lines of 9, 10, 11, 12 and 15 fields, CRLF, a .gz copy,
fields of 1 to 10 digits, fields that are no numbers; with 1, 2 and 7 worker threads, below and above the size from which the text
is tokenised in chunks.  The six ordinary columns and the symmetric flag are those of the plain parser on the same text."""
import gzip
import re

import numpy as np
import pytest
from raft_testlib import write_fasta

from raft_amd import hostio

N_READS = 40
NAMES = [f"read_{i}/ccs" for i in range(N_READS)]
ODD_FIELDS = ["", "abc", "12x", "-5", "+3", " 7", "x9", "0", "007", "99999999999999999999", "-99999999999999999999", "4294967295", "2147483648"]


def c_num(s: str) -> int:
    """The tokeniser's number (paf.hpp:64-75 -> chop.hpp:157-160): strtol, then uint32, then int."""
    m = re.match(r"[ \t\n\v\f\r]*([+-]?)(\d*)", s)
    if not m.group(2):
        return 0
    v = int(m.group(2)) * (-1 if m.group(1) == "-" else 1)
    v = max(min(v, 2 ** 63 - 1), -2 ** 63) & 0xFFFFFFFF
    return v - 2 ** 32 if v >= 2 ** 31 else v


def restate(text: str):
    """-> eight lists: qid, qs, qe, tid, ts, te, matches, block of every line with ten fields or more."""
    index = {n: i for i, n in enumerate(NAMES)}
    rows = []
    for line in text.split("\n"):
        if len(line) > 1 and line.endswith("\r"):
            line = line[:-1]
        f = line.split("\t")
        if len(f) < 10:
            continue
        rows.append((index[f[0]], c_num(f[2]), c_num(f[3]), index[f[5]], c_num(f[7]), c_num(f[8]), c_num(f[9]), c_num(f[10]) if len(f) >= 11 else 0))
    return [np.array([r[k] for r in rows], np.int32) for k in range(8)]


def digits(rng, n):
    return str(int(rng.integers(1, 10))) + "".join(str(int(d)) for d in rng.integers(0, 10, n - 1))


def make_text(n_lines: int, seed: int, eol: str = "\n", mirror_first: bool = False, last_newline: bool = True) -> str:
    rng = np.random.default_rng(seed)
    tail = ["60", "tp:A:P", "cm:i:100", "s1:i:90", "dv:f:0.01", "rl:i:0"]
    lines = []
    for i in range(n_lines):
        n_fields = (11, 12, 15, 10, 9, 12)[i % 6] if i else 12
        a, b = int(rng.integers(0, N_READS)), int(rng.integers(0, N_READS))
        coord = [digits(rng, int(rng.integers(1, 8))) for _ in range(4)]
        quality = [digits(rng, 1 + (i + k) % 10) for k in range(2)]
        if i % 11 == 5:
            quality[i // 11 % 2] = ODD_FIELDS[i // 22 % len(ODD_FIELDS)]
        if i % 97 == 13:
            coord[i % 4] = digits(rng, 10)
        f = [NAMES[a], "20000", coord[0], coord[1], "+-"[i % 2], NAMES[b], "25000", coord[2], coord[3]] + quality + tail
        lines.append("\t".join(f[:n_fields]))
    if mirror_first:
        f = lines[0].split("\t")
        lines.insert(n_lines // 2, "\t".join([f[5], f[6], f[7], f[8], f[4], f[0], f[1], f[2], f[3]] + f[9:11]))
    return eol.join(lines) + (eol if last_newline else "")


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    d = tmp_path_factory.mktemp("quality_reads")
    write_fasta(d / "reads.fa", NAMES, [50] * N_READS)
    r = hostio.Reads(str(d / "reads.fa"))
    yield r
    r.close()
    hostio.set_threads(0)


def compare(path, text, reads, what):
    want = restate(text)
    plain, flag = hostio.load_paf(str(path), reads, with_flag=True)
    for two_steps in (False, True):
        got, qflag = hostio.load_paf(str(path), reads, with_flag=True, two_steps=two_steps, quality=True)
        assert len(got) == 8 and all(c.dtype == np.int32 for c in got)
        for k in range(8):
            bad = np.flatnonzero(got[k] != want[k]) if got[k].shape == want[k].shape else None
            assert bad is not None and bad.size == 0, (what, two_steps, k, got[k].shape, want[k].shape, None if bad is None else (bad[0], got[k][bad[0]], want[k][bad[0]]))
        assert all(np.array_equal(a, b) for a, b in zip(got[:6], plain)) and qflag == flag, (what, two_steps)
    return want, flag


@pytest.mark.parametrize("threads", [1, 2, 7])
@pytest.mark.parametrize("n_lines", [300, 30000], ids=["one chunk", "chunks"])
def test_the_two_columns_equal_a_python_split(tmp_path, reads, threads, n_lines):
    hostio.set_threads(threads)
    text = make_text(n_lines, seed=n_lines)
    assert (len(text) > (1 << 20)) == (n_lines == 30000)              # host_io.cpp: a text below 1 MiB is one chunk
    (tmp_path / "a.paf").write_text(text)
    want, flag = compare(tmp_path / "a.paf", text, reads, "plain")
    assert flag == 0 and want[0].size == n_lines - n_lines // 6          # every sixth line has nine fields
    ten = np.array([i % 6 == 3 for i in range(n_lines) if i % 6 != 4])
    assert np.all(want[7][ten] == 0) and np.any(want[7][~ten] != 0)      # ten fields: block is 0
    with gzip.open(tmp_path / "a.paf.gz", "wt", newline="") as f:
        f.write(text)
    compare(tmp_path / "a.paf.gz", text, reads, "gz")
    crlf = make_text(n_lines, seed=n_lines, eol="\r\n")
    (tmp_path / "crlf.paf").write_bytes(crlf.encode())
    got, _ = compare(tmp_path / "crlf.paf", crlf, reads, "crlf")
    assert all(np.array_equal(a, b) for a, b in zip(got, want))          # the carriage return belongs to no field
    mirrored = make_text(n_lines, seed=n_lines, mirror_first=True, last_newline=False)
    (tmp_path / "m.paf").write_text(mirrored)
    _, flag = compare(tmp_path / "m.paf", mirrored, reads, "mirror of the first record, no last newline")
    assert flag == 1


def test_the_odd_fields_are_all_there():
    """(what the generated text is for: every odd field in either column, all digit counts, ten-field lines)"""
    text = make_text(3000, seed=3000)
    rows = [ln.split("\t") for ln in text.split("\n") if ln.count("\t") >= 9]
    for k in (9, 10):
        fields = {r[k] for r in rows if len(r) > k}
        assert set(ODD_FIELDS) <= fields and {len(f) for f in fields if f.isdigit()} >= set(range(1, 11))
    assert {len(r) for r in rows} == {10, 11, 12, 15}
    assert [c_num(s) for s in ("", "abc", "12x", "-5", "+3", " 7", "4294967295", "2147483648", "99999999999999999999")] == [0, 0, 12, -5, 3, 7, -1, -2 ** 31, -1]


def test_an_object_parsed_without_the_columns_has_none(tmp_path, reads):
    import ctypes as C
    lib = hostio.load_library()
    (tmp_path / "a.paf").write_text(make_text(50, seed=1))
    for fn, has in ((lib.raft_host_paf_load, False), (lib.raft_host_paf_load_quality, True)):
        h = C.c_void_p()
        assert fn(str(tmp_path / "a.paf").encode(), reads._h, C.byref(h), None, 0) == hostio.OK
        assert [bool(lib.raft_host_paf_quality(h, k)) for k in (0, 1)] == [has, has]
        assert not lib.raft_host_paf_quality(h, 2) and not lib.raft_host_paf_quality(h, -1) and not lib.raft_host_paf_quality(None, 0)
        lib.raft_host_paf_free(h)


def test_a_dropped_line_with_an_unknown_name_is_still_an_error(tmp_path, reads):
    text = make_text(20, seed=2) + "\t".join(["nobody", "1", "0", "1", "+", NAMES[0], "1", "0", "1", "0", "0"]) + "\n"
    (tmp_path / "a.paf").write_text(text)
    with pytest.raises(hostio.HostError) as e:
        hostio.load_paf(str(tmp_path / "a.paf"), reads, quality=True)
    assert e.value.code == hostio.ERR_UNKNOWN_NAME and e.value.what == "nobody"
