"""CPU: raft_host_write_repeat_overlaps (PREFIX.repeat_overlaps.tsv and PREFIX.repeat_overlaps.records.tsv of `raft --repeat-overlaps`)
against literal text, against a restatement of its two line formats, and under 1, 2 and 7 worker threads."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
from raft_testlib import ROOT


def restate_reads(names, length, touch, repeat, flags):
    """One line per read: name, length, sides touching a repeat, sides inside one, contained: no / anchored / repeat."""
    word = lambda f: "no" if not f & 1 else "anchored" if f & 2 else "repeat"
    return "".join(f"{n}\t{int(l)}\t{int(t)}\t{int(r)}\t{word(int(f))}\n" for n, l, t, r, f in zip(names, length, touch, repeat, flags))


def restate_records(names, qid, qs, qe, tid, ts, te, cls):
    """One line per record with a side inside a repeat (class & 3), in record order."""
    out = []
    for i in np.flatnonzero(np.asarray(cls) & 3):
        c = int(cls[i])
        side = "both" if c & 3 == 3 else "query" if c & 1 else "target"
        contained = "query" if c & 16 else "target" if c & 32 else "-"
        t = ("-", "-") if ts is None else (int(ts[i]), int(te[i]))
        out.append(f"{names[qid[i]]}\t{int(qs[i])}\t{int(qe[i])}\t{names[tid[i]]}\t{t[0]}\t{t[1]}\t{side}\t{contained}\n")
    return "".join(out)


def write(lib, reads_path, records_path, names, length, touch, repeat, flags, cols, cls):
    arr = (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
    P = lambda a: C.c_void_p(0 if a is None or a.size == 0 else a.ctypes.data)
    S = lambda p: None if p is None else str(p).encode()
    keep = [None if a is None else np.ascontiguousarray(a) for a in [length, touch, repeat, flags] + list(cols) + [cls]]
    return lib.raft_host_write_repeat_overlaps(S(reads_path), S(records_path), len(names), arr, *[P(a) for a in keep[:4]], cols[0].size,
                                               *[P(a) for a in keep[4:]])


NAMES = ["r0", "read/1 with_odd-chars|x=1", "x", "longest"]
LENGTH = np.array([5000, 9000, 1, 2147483647], np.int32)
TOUCH, REPEAT = np.array([0, 3, 7, 2147483647], np.int32), np.array([0, 1, 7, 12], np.int32)
FLAGS = np.array([0, 3, 1, 2], np.uint8)              # (2 alone: an anchor without containment cannot arise; it reads "no")
COLS = [np.array(v, np.int32) for v in ([0, 1, 2, 3, 0, 1], [0, 10, 0, 5, 7, 2147483000], [5000, 20, 1, 6, 8, 2147483647], [1, 0, 3, 2, 0, 3],
                                         [100, 0, -3, 0, 1, 2], [5100, 5000, 4, 1, 2, 3])]
CLS = np.array([16 | 10 | 5, 4 | 32 | 1, 8 | 2, 12, 0, 3], np.uint8)
READS_TEXT = ("r0\t5000\t0\t0\tno\n" "read/1 with_odd-chars|x=1\t9000\t3\t1\tanchored\n" "x\t1\t7\t7\trepeat\n" "longest\t2147483647\t2147483647\t12\tno\n")
RECORDS_TEXT = ("r0\t0\t5000\tread/1 with_odd-chars|x=1\t100\t5100\tboth\tquery\n"
                "read/1 with_odd-chars|x=1\t10\t20\tr0\t0\t5000\tquery\ttarget\n"
                "x\t0\t1\tlongest\t-3\t4\ttarget\t-\n"
                "read/1 with_odd-chars|x=1\t2147483000\t2147483647\tlongest\t2\t3\tboth\t-\n")


def test_host_writer_against_literal_text(tmp_path):
    from raft_amd import hostio
    lib = hostio.load_library()
    a, b = tmp_path / "reads.tsv", tmp_path / "records.tsv"
    assert write(lib, a, b, NAMES, LENGTH, TOUCH, REPEAT, FLAGS, COLS, CLS) == 0
    assert open(a).read() == READS_TEXT == restate_reads(NAMES, LENGTH, TOUCH, REPEAT, FLAGS)
    assert open(b).read() == RECORDS_TEXT == restate_records(NAMES, *COLS, CLS)
    # without target coordinates: "-" for both
    assert write(lib, None, b, NAMES, LENGTH, TOUCH, REPEAT, FLAGS, COLS[:4] + [None, None], CLS) == 0
    assert open(b).read() == restate_records(NAMES, *COLS[:4], None, None, CLS) and "\tr0\t-\t-\tquery\ttarget\n" in open(b).read()
    # one table alone
    os.remove(b)
    assert write(lib, a, None, NAMES, LENGTH, TOUCH, REPEAT, FLAGS, COLS, CLS) == 0 and not os.path.exists(b)
    # an unwritable path; a listed record that names a read outside the table
    assert write(lib, tmp_path / "no_such_dir" / "x.tsv", b, NAMES, LENGTH, TOUCH, REPEAT, FLAGS, COLS, CLS) != 0
    bad = [c.copy() for c in COLS]
    bad[3][0] = 4
    assert write(lib, a, b, NAMES, LENGTH, TOUCH, REPEAT, FLAGS, bad, CLS) != 0
    bad[3][0] = 1; bad[0][4] = -1                                                 # (record 4 is not listed: its ids are not looked at)
    assert write(lib, a, b, NAMES, LENGTH, TOUCH, REPEAT, FLAGS, bad, CLS) == 0 and open(b).read() == RECORDS_TEXT


def test_no_reads_and_no_listed_records(tmp_path):
    from raft_amd import hostio
    lib = hostio.load_library()
    a, b = tmp_path / "reads.tsv", tmp_path / "records.tsv"
    none = np.empty(0, np.int32)
    assert write(lib, a, b, [], none, none, none, np.empty(0, np.uint8), [none] * 6, np.empty(0, np.uint8)) == 0
    assert open(a).read() == "" and open(b).read() == ""
    assert write(lib, a, b, NAMES, LENGTH, TOUCH, REPEAT, FLAGS, COLS, CLS & 0xFC) == 0         # touching and contained, none inside
    assert open(a).read() == READS_TEXT and open(b).read() == ""
    assert write(lib, a, b, NAMES, LENGTH, TOUCH, REPEAT, FLAGS, [none] * 6, np.empty(0, np.uint8)) == 0
    assert open(a).read() == READS_TEXT and open(b).read() == ""


_CHILD = r"""
import hashlib, sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import numpy as np
from raft_amd import hostio
from test_repeat_overlaps_writer import restate_reads, restate_records, write
rng = np.random.default_rng(4)
n_reads, n_rec = 9001, 40003                     # several blocks of lines for every worker, and a last short one
names = [f"read_{i}/{i * 7919 % 1000}" for i in range(n_reads)]
length = rng.integers(1, 2**31 - 1, n_reads).astype(np.int32)
touch, repeat = rng.integers(0, 10**6, n_reads).astype(np.int32), rng.integers(0, 50, n_reads).astype(np.int32)
flags = rng.integers(0, 4, n_reads).astype(np.uint8)
cols = [rng.integers(0, n_reads, n_rec).astype(np.int32) if k in (0, 3) else rng.integers(-5, 2**31 - 1, n_rec).astype(np.int32) for k in range(6)]
cls = rng.integers(0, 64, n_rec).astype(np.uint8)
cls[20000:33000] &= 0xFC                        # (whole blocks without a listed record)
assert write(hostio.load_library(), sys.argv[2], sys.argv[3], names, length, touch, repeat, flags, cols, cls) == 0
assert open(sys.argv[2]).read() == restate_reads(names, length, touch, repeat, flags)
assert open(sys.argv[3]).read() == restate_records(names, *cols, cls)
print(hashlib.md5(open(sys.argv[2], "rb").read()).hexdigest(), hashlib.md5(open(sys.argv[3], "rb").read()).hexdigest())
"""


def test_the_bytes_do_not_depend_on_the_threads(tmp_path):
    """The thread count is read once per process (RAFT_HOST_THREADS, RAFT_FORMAT_THREADS): one process per count, the same data."""
    seen = set()
    for threads in (1, 2, 7):
        env = dict(os.environ, RAFT_HOST_THREADS=str(threads), RAFT_FORMAT_THREADS=str(threads))
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(tmp_path / f"a{threads}.tsv"), str(tmp_path / f"b{threads}.tsv")], env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        seen.add(r.stdout.strip())
    assert len(seen) == 1 and len(seen.pop().split()) == 2
