"""CPU: raft_host_write_low_coverage (PREFIX.low_coverage.bed of `raft --low-cov`) against a restatement of its line format."""
import ctypes as C

import numpy as np


def restate_bed(names, low_offset, low_s, low_e, read_len):
    """One line per run, in read order: name, start, end, class -- whole (from base 0 to the read's length), head, tail or interior."""
    out = []
    for i, nm in enumerate(names):
        for k in range(int(low_offset[i]), int(low_offset[i + 1])):
            head, tail = int(low_s[k]) == 0, int(low_e[k]) == int(read_len[i])
            out.append(f"{nm}\t{int(low_s[k])}\t{int(low_e[k])}\t{'whole' if head and tail else 'head' if head else 'tail' if tail else 'interior'}\n")
    return "".join(out)


def _write(lib, path, names, off, s, e, rl, reso):
    arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
    P = lambda a: C.c_void_p(a.ctypes.data if a.size else 0)
    return lib.raft_host_write_low_coverage(str(path).encode(), len(names), arr, P(off), P(s), P(e), P(rl), reso)


def test_host_writer_against_the_line_format(tmp_path):
    from raft_amd import hostio
    lib = hostio.load_library()
    names = ["r0", "read/1 with_odd-chars|x=1", "x", "empty", "one"]
    for reso in (50, 1, 1000):
        rl = np.array([20 * reso - 7 if reso > 7 else 20, 3 * reso, 2147483647, 0, 1], np.int32)
        off = np.array([0, 3, 4, 6, 6, 7], np.int64)
        s = np.array([0, 5 * reso, 18 * reso, 0, reso, 2147483647 - 5, 0], np.int32)
        e = np.array([2 * reso, 6 * reso, rl[0], rl[1], 2 * reso, 2147483647, 1], np.int32)
        path = tmp_path / f"t{reso}.bed"
        assert _write(lib, path, names, off, s, e, rl, reso) == 0
        text = open(path).read()
        assert text == restate_bed(names, off, s, e, rl)
        assert [ln.split("\t")[3] for ln in text.splitlines()] == ["head", "interior", "tail", "whole", "interior", "tail", "whole"]
    assert _write(lib, tmp_path / "no_such_dir" / "x.bed", names, off, s, e, rl, 50) != 0          # an unwritable path
    assert _write(lib, tmp_path / "bad.bed", names, off, s, e, rl, 0) != 0                          # reso must be positive


def test_no_runs_and_no_reads(tmp_path):
    from raft_amd import hostio
    lib = hostio.load_library()
    none = np.empty(0, np.int32)
    assert _write(lib, tmp_path / "a.bed", ["a", "b"], np.zeros(3, np.int64), none, none, np.array([10, 20], np.int32), 50) == 0
    assert open(tmp_path / "a.bed").read() == ""
    assert _write(lib, tmp_path / "b.bed", [], np.zeros(1, np.int64), none, none, none, 50) == 0
    assert open(tmp_path / "b.bed").read() == ""
