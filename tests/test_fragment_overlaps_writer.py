"""CPU: raft_host_write_fragments (PREFIX.fragments.tsv of `raft --fragment-overlaps`) against literal text, against a restatement of its
line format, and under 1, 2 and 7 worker threads."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
from raft_testlib import ROOT


def restate(names, frag_offset, begin, end, touch, span, contained, repeat):
    """One line per fragment row in row order: the row's number from 1, the name of its read, then the six integers."""
    out = []
    for r, name in enumerate(names):
        for k in range(int(frag_offset[r]), int(frag_offset[r + 1])):
            out.append(f"{k + 1}\t{name}\t{int(begin[k])}\t{int(end[k])}\t{int(touch[k])}\t{int(span[k])}\t{int(contained[k])}\t{int(repeat[k])}\n")
    return "".join(out)


def write(lib, path, names, frag_offset, *cols):
    arr = (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
    P = lambda a: C.c_void_p(0 if a is None or a.size == 0 else a.ctypes.data)
    keep = [None if a is None else np.ascontiguousarray(a) for a in (frag_offset,) + cols]
    return lib.raft_host_write_fragments(None if path is None else str(path).encode(), len(names), arr, *[P(a) for a in keep])


NAMES = ["r0", "read/1 with_odd-chars|x=1", "none", "longest"]
OFFSET = np.array([0, 2, 3, 3, 5], np.int64)
COLS = [np.array(v, np.int32) for v in ([0, 3500, 0, 7, 7], [4000, 9000, 1, 7, 2147483647], [3, 0, 12, 0, 2147483647], [2, 0, 12, 0, 5],
                                        [1, 0, 0, 0, 5], [2000, 0, 1, 0, 2147483640])]
TEXT = ("1\tr0\t0\t4000\t3\t2\t1\t2000\n" "2\tr0\t3500\t9000\t0\t0\t0\t0\n" "3\tread/1 with_odd-chars|x=1\t0\t1\t12\t12\t0\t1\n"
        "4\tlongest\t7\t7\t0\t0\t0\t0\n" "5\tlongest\t7\t2147483647\t2147483647\t5\t5\t2147483640\n")


def test_host_writer_against_literal_text(tmp_path):
    from raft_amd import hostio
    lib = hostio.load_library()
    a = tmp_path / "fragments.tsv"
    assert write(lib, a, NAMES, OFFSET, *COLS) == 0
    assert open(a).read() == TEXT == restate(NAMES, OFFSET, *COLS)
    # an unwritable path, no path, offsets that do not begin at 0 or step back, a missing column
    assert write(lib, tmp_path / "no_such_dir" / "x.tsv", NAMES, OFFSET, *COLS) != 0
    assert write(lib, None, NAMES, OFFSET, *COLS) != 0
    os.remove(a)
    assert write(lib, a, NAMES, np.array([1, 2, 3, 3, 5], np.int64), *COLS) != 0
    assert write(lib, a, NAMES, np.array([0, 2, 1, 3, 5], np.int64), *COLS) != 0
    assert write(lib, a, NAMES, OFFSET, *COLS[:5], None) != 0
    assert not os.path.exists(a)


def test_no_reads_and_no_rows(tmp_path):
    from raft_amd import hostio
    lib = hostio.load_library()
    a = tmp_path / "fragments.tsv"
    none = np.empty(0, np.int32)
    assert write(lib, a, [], np.zeros(1, np.int64), *[none] * 6) == 0 and open(a).read() == ""
    assert write(lib, a, NAMES, np.zeros(5, np.int64), *[none] * 6) == 0 and open(a).read() == ""


_CHILD = r"""
import hashlib, sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import numpy as np
from raft_amd import hostio
from test_fragment_overlaps_writer import restate, write
rng = np.random.default_rng(4)
n_reads = 30011                                  # several blocks of reads for every worker, and a last short one
count = rng.integers(0, 5, n_reads)
count[1000:9000] = 0                             # (whole blocks without a row)
count[12345] = 20000                             # (one read heavier than a block)
offset = np.zeros(n_reads + 1, np.int64)
offset[1:] = np.cumsum(count)
names = [f"read_{i}/{i * 7919 % 1000}" for i in range(n_reads)]
cols = [rng.integers(0, 2**31 - 1, int(offset[-1])).astype(np.int32) for _ in range(6)]
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
