"""CPU: raft_host_write_repeat_stats (PREFIX.long_repeats.stats.tsv of `raft --repeat-stats`) against literal text, against a Python
formatter of its line format, with each of the five `where` values, with bad offsets, and under 1, 2 and 7 worker threads."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
from raft_testlib import ROOT

WHERE = {0: "interior", 2: "head", 4: "tail", 6: "whole", 1: "empty", 3: "empty", 5: "empty", 7: "empty"}


def restate(names, rep_offset, s, e, flags, windows, cov_sum, cov_min, cov_max, high, touch, span, inside):
    """One line per run, read by read: name, start, end, where, then the eight integers."""
    out = []
    for r, name in enumerate(names):
        for k in range(int(rep_offset[r]), int(rep_offset[r + 1])):
            nums = "\t".join(str(int(c[k])) for c in (windows, cov_sum, cov_min, cov_max, high, touch, span, inside))
            out.append(f"{name}\t{int(s[k])}\t{int(e[k])}\t{WHERE[int(flags[k])]}\t{nums}\n")
    return "".join(out)


def write(lib, path, names, rep_offset, *cols):
    arr = (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
    P = lambda a: C.c_void_p(0 if a is None or a.size == 0 else a.ctypes.data)
    keep = [None if a is None else np.ascontiguousarray(a) for a in (rep_offset,) + cols]
    return lib.raft_host_write_repeat_stats(None if path is None else str(path).encode(), len(names), arr, *[P(a) for a in keep])


NAMES = ["r0", "read/1 with_odd-chars|x=1", "none", "longest"]
OFFSET = np.array([0, 2, 3, 3, 6], np.int64)
_I = lambda *v: np.array(v, np.int32)
COLS = [_I(1000, 3500, 0, 0, 7, -5), _I(4000, 9000, 800, 9000, 7, 2147483647), np.array([0, 4, 2, 6, 1, 7], np.uint8), _I(60, 110, 16, 180, 0, 2147483647),
        np.array([1234, 0, 99, 2**40, 0, -1], np.int64), _I(3, 0, 1, 2, 0, 5), _I(40, 0, 9, 2147483647, 0, 6), _I(7, 0, 0, 180, 0, 1),
        _I(12, 0, 3, 2147483647, 0, 2), _I(2, 0, 1, 5, 0, 3), _I(1, 0, 0, 2147483640, 0, 4)]
TEXT = ("r0\t1000\t4000\tinterior\t60\t1234\t3\t40\t7\t12\t2\t1\n" "r0\t3500\t9000\ttail\t110\t0\t0\t0\t0\t0\t0\t0\n"
        "read/1 with_odd-chars|x=1\t0\t800\thead\t16\t99\t1\t9\t0\t3\t1\t0\n"
        "longest\t0\t9000\twhole\t180\t1099511627776\t2\t2147483647\t180\t2147483647\t5\t2147483640\n" "longest\t7\t7\tempty\t0\t0\t0\t0\t0\t0\t0\t0\n"
        "longest\t-5\t2147483647\tempty\t2147483647\t-1\t5\t6\t1\t2\t3\t4\n")


def test_host_writer_against_literal_text(tmp_path):
    from raft_amd import hostio
    lib = hostio.load_library()
    a = tmp_path / "stats.tsv"
    assert write(lib, a, NAMES, OFFSET, *COLS) == 0
    assert open(a).read() == TEXT == restate(NAMES, OFFSET, *COLS)
    assert {ln.split("\t")[3] for ln in TEXT.splitlines()} == {"interior", "head", "tail", "whole", "empty"}
    # an unwritable path, no path, offsets that do not begin at 0 or step back, a missing column (each in turn)
    assert write(lib, tmp_path / "no_such_dir" / "x.tsv", NAMES, OFFSET, *COLS) != 0
    assert write(lib, None, NAMES, OFFSET, *COLS) != 0
    os.remove(a)
    assert write(lib, a, NAMES, np.array([1, 2, 3, 3, 6], np.int64), *COLS) != 0
    assert write(lib, a, NAMES, np.array([0, 2, 1, 3, 6], np.int64), *COLS) != 0
    for k in range(len(COLS)):
        assert write(lib, a, NAMES, OFFSET, *COLS[:k], None, *COLS[k + 1:]) != 0, k
    assert not os.path.exists(a)


def test_every_flag_byte_has_its_word(tmp_path):
    from raft_amd import hostio
    a = tmp_path / "stats.tsv"
    z = np.zeros(8, np.int32)
    cols = [z, z, np.arange(8, dtype=np.uint8), z, np.zeros(8, np.int64)] + [z] * 6
    assert write(hostio.load_library(), a, ["x"], np.array([0, 8], np.int64), *cols) == 0
    assert [ln.split("\t")[3] for ln in open(a).read().splitlines()] == [WHERE[f] for f in range(8)]


def test_no_reads_and_no_runs(tmp_path):
    from raft_amd import hostio
    lib = hostio.load_library()
    a = tmp_path / "stats.tsv"
    none = np.empty(0, np.int32)
    assert write(lib, a, [], np.zeros(1, np.int64), *[none] * 11) == 0 and open(a).read() == ""
    assert write(lib, a, NAMES, np.zeros(5, np.int64), *[none] * 11) == 0 and open(a).read() == ""


_CHILD = r"""
import hashlib, sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import numpy as np
from raft_amd import hostio
from test_repeat_stats_writer import restate, write
rng = np.random.default_rng(4)
n_reads = 30011                                  # several blocks of reads for every worker, and a last short one
count = rng.integers(0, 5, n_reads)
count[1000:9000] = 0                             # (whole blocks without a run)
count[12345] = 20000                             # (one read heavier than a block)
offset = np.zeros(n_reads + 1, np.int64)
offset[1:] = np.cumsum(count)
names = [f"read_{i}/{i * 7919 % 1000}" for i in range(n_reads)]
n = int(offset[-1])
cols = [rng.integers(-5, 2**31 - 1, n).astype(np.int32) for _ in range(11)]
cols[2] = rng.integers(0, 8, n).astype(np.uint8)
cols[4] = rng.integers(0, 2**50, n).astype(np.int64)
assert write(hostio.load_library(), sys.argv[2], names, offset, *cols) == 0
assert open(sys.argv[2]).read() == restate(names, offset, *cols)
print(hashlib.md5(open(sys.argv[2], "rb").read()).hexdigest())
"""


def test_the_bytes_do_not_depend_on_the_threads(tmp_path):
    """The thread count is read once per process (RAFT_HOST_THREADS, RAFT_FORMAT_THREADS): one process per count, the same data."""
    seen = set()
    for threads in (1, 2, 7):
        env = dict(os.environ, RAFT_HOST_THREADS=str(threads), RAFT_FORMAT_THREADS=str(threads))
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(tmp_path / f"a{threads}.tsv")], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        seen.add(r.stdout.strip())
    assert len(seen) == 1 and len(seen.pop()) == 32
