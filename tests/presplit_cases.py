"""The sets that put the pre-split job (raft_hip_run_presplit_local and what it is made of: raft_hip_presplit_symmetric_local,
raft_hip_group_sides, raft_hip_exchange_local) on its structural edges, and a plain-Python model of the job's two cut rules.

A case is tiny: a handful of reads, a handful of records, a number of ranks.  What it is FOR is written beside it twice: the classes
it claims to fill (CLASSES: the census of tests/test_presplit_cases.py fails on an empty one) and what the two cuts make of it --
which ranks own no reads, which slices are empty, which ranks receive nothing, how many runs arrive at every rank.  Both are literals
here and are checked against the model there, so a case that stops reaching its edge (a changed cut rule, an edited stream) fails on
the CPU instead of quietly testing something else on the GPU.

Nothing here needs a device."""
from __future__ import annotations

from bisect import bisect_left

import numpy as np
from raft_testlib import RaftParams, oracle_run

RESO = 50
P30 = RaftParams(est_cov=30)
# repeats and fragments on short reads: two high windows are a repeat (the capacities of tests/test_gpu_presplit_edges.py need
# repeats and fragments on ranks other than the first)
P_SHORT = RaftParams(est_cov=30, repeat_length=100, interval_length=100, read_length=300, overlap_length=20, flanking_length=50)

FIELDS = ("qid", "qs", "qe", "tid", "ts", "te")


def mirror(r):
    """The record with query and target swapped (chop.hpp:175-184 compares record i with this of record 0)."""
    return (r[3], r[4], r[5], r[0], r[1], r[2])


# ---- the model: the job's two cut rules, restated ---------------------------------------------------------------------------

def record_cut(n_rec: int, world: int) -> list:
    """Rank r holds records [cut[r], cut[r + 1]) of the stream."""
    return [n_rec * r // world for r in range(world + 1)]


def window_prefix(read_len, reso: int) -> list:
    off = [0]
    for ln in read_len:
        off.append(off[-1] + (int(ln) + reso - 1) // reso)
    return off


def read_bounds(read_len, reso: int, world: int) -> list:
    """Rank g owns reads [bounds[g], bounds[g + 1]): the first read at which the window prefix sum reaches W g / world."""
    off = window_prefix(read_len, reso)
    W, n_reads = off[-1], len(off) - 1
    b = [0] * (world + 1)
    for g in range(1, world):
        b[g] = bisect_left(off, W * g // world)
    b[world] = n_reads
    for g in range(1, world + 1):
        b[g] = min(max(b[g], b[g - 1]), n_reads)
    return b


def stream_symmetric(recs) -> bool:
    return any(tuple(r) == mirror(recs[0]) for r in recs[1:])


def sides_of(recs, symmetric: bool) -> list:
    """(record index, read) of every interval the job piles up: query sides, and target sides on another read unless symmetric."""
    out = []
    for i, r in enumerate(recs):
        out.append((i, r[0]))
        if not symmetric and r[3] != r[0]:
            out.append((i, r[3]))
    return out


class Model:
    """What the two cuts make of a case."""

    def __init__(self, case):
        w = case.world
        self.cut = record_cut(len(case.recs), w)
        self.prefix = window_prefix(case.read_len, case.p.reso)
        self.bounds = read_bounds(case.read_len, case.p.reso, w)
        self.symmetric = stream_symmetric(case.recs) if case.recs else False
        self.no_reads = {g for g in range(w) if self.bounds[g] == self.bounds[g + 1]}
        self.empty_slices = {r for r in range(w) if self.cut[r] == self.cut[r + 1]}
        owner = {}
        for g in range(w):
            for read in range(self.bounds[g], self.bounds[g + 1]):
                owner[read] = g
        pieces = [set() for _ in range(w)]                  # per rank: the slices with an interval for one of its reads
        self.n_intervals = [0] * w
        for i, read in sides_of(case.recs, self.symmetric):
            sl = max(r for r in range(w) if self.cut[r] <= i)
            pieces[owner[read]].add(sl)
            self.n_intervals[owner[read]] += 1
        self.runs = [len(s) for s in pieces]               # (a slice is ONE sorted run once its sides are grouped)
        self.receives_nothing = {g for g in range(w) if not pieces[g]}
        self.mirror_slice = None
        if self.symmetric:
            i = next(i for i, r in enumerate(case.recs) if i > 0 and tuple(r) == mirror(case.recs[0]))
            self.mirror_index = i
            self.mirror_slice = max(r for r in range(w) if self.cut[r] <= i)
        self.first_slice = min((r for r in range(w) if r not in self.empty_slices), default=None)


class PresplitCase:
    def __init__(self, name, world, read_len, recs, classes, no_reads, empty_slices, receives_nothing, runs, symmetric, p=P30, widths=(1,)):
        self.name, self.world, self.p, self.widths = name, world, p, tuple(widths)
        self.read_len = np.asarray(read_len, np.int32).reshape(-1)
        self.recs = [tuple(int(x) for x in r) for r in recs]
        self.classes = frozenset(classes) | {f"world={world}"}
        self.no_reads, self.empty_slices, self.receives_nothing = set(no_reads), set(empty_slices), set(receives_nothing)
        self.runs, self.symmetric = list(runs), int(symmetric)
        self._want = None

    @property
    def cols(self):
        """The six int32 columns."""
        a = np.asarray(self.recs, np.int32).reshape(-1, 6)
        return [np.ascontiguousarray(a[:, k]) for k in range(6)]

    @property
    def n_rec(self):
        return len(self.recs)

    def oracle(self):
        """The oracle's outputs for the whole set (computed once, never written to)."""
        if self._want is None:
            self._want = oracle_run(self.p, self.read_len, *self.cols)
            for v in self._want.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        return self._want

    def __repr__(self):
        return self.name


# ---- streams ------------------------------------------------------------------------------------------------------------------

def _span(a, b, ln):
    s = (37 * a + 91 * b) % (ln // 2)
    return s, s + 1 + (53 * a + 17 * b) % (ln // 2)


def pair(a, b, lens):
    """The overlap of reads a and b as a's record: pair(b, a) is its mirror."""
    return (a, *_span(a, b, lens[a]), b, *_span(b, a, lens[b]))


def all_vs_all(lens, half=False):
    n = len(lens)
    return [pair(a, b, lens) for a in range(n) for b in range(n) if a != b and (not half or a < b)]


def shuffled(recs, step):
    """A fixed permutation that keeps record 0 in front (the flag is about record 0)."""
    n = len(recs)
    assert np.gcd(step, n) == 1
    return [recs[i * step % n] for i in range(n)]


A_B = (0, 100, 600, 1, 200, 700)
NEAR = {0: (2, 200, 700, 0, 100, 600), 1: (1, 201, 700, 0, 100, 600), 2: (1, 200, 701, 0, 100, 600),
        3: (1, 200, 700, 2, 100, 600), 4: (1, 200, 700, 0, 101, 600), 5: (1, 200, 700, 0, 100, 601)}
SELF = [(0, 100, 600, 0, 100, 600), (0, 0, 300, 0, 500, 800), (0, 200, 900, 0, 300, 1000), (0, 50, 150, 0, 700, 800)]
CHAIN = [(0, 100, 600, 1, 200, 700), (1, 0, 500, 2, 300, 800), (2, 100, 300, 0, 600, 800), (0, 400, 900, 2, 50, 550)]
DEEP = [(1, 0, 100, 1, 0, 100)] * 260 + [(3, 50, 150, 3, 50, 150)] * 256
K3, K16 = [1000] * 3, [1000] * 16


def _build():
    C = PresplitCase
    cases = [
        # -- the record cut
        C("no_records/w3", 3, K3, [], {"n_rec=0"}, set(), {0, 1, 2}, {0, 1, 2}, [0, 0, 0], 0),
        C("one_record/w3", 3, K3, [A_B], {"n_rec=1", "n_rec<world, no mirror/w3", "owner receives nothing", "non-symmetric"},
          set(), {0, 1}, {2}, [1, 1, 0], 0),
        C("mirrored_pair/w3", 3, [1000, 1000], [A_B, mirror(A_B)],
          {"n_rec=world-1", "n_rec<world, mirror in a later slice/w3", "n_reads<world", "mirror last of the last rank"},
          {2}, {0}, {2}, [1, 1, 0], 1),
        C("mirrored_pair/w8", 8, [1000, 1000], [A_B, mirror(A_B)],
          {"n_rec<world, mirror in a later slice/w8", "n_reads<world", "mirror last of the last rank"},
          {1, 2, 3, 5, 6, 7}, {0, 1, 2, 4, 5, 6}, {1, 2, 3, 5, 6, 7}, [1, 0, 0, 0, 1, 0, 0, 0], 1),
        C("half_of_the_pair/w8", 8, [1000, 1000], [A_B], {"n_rec=1", "n_rec<world, no mirror/w8", "n_reads<world", "non-symmetric"},
          {1, 2, 3, 5, 6, 7}, {0, 1, 2, 3, 4, 5, 6}, {1, 2, 3, 5, 6, 7}, [1, 0, 0, 0, 1, 0, 0, 0], 0),
        # (rank 0 owns NO read here: W / 64 rounds to 0, and the first read's prefix sum is the first to reach it)
        C("mirrored_pair/w64", 64, [1000, 1000], [A_B, mirror(A_B)], {"n_reads<world", "mirror last of the last rank"},
          set(range(64)) - {1, 33}, set(range(64)) - {31, 63}, set(range(64)) - {1, 33}, [int(g in (1, 33)) for g in range(64)], 1),
        C("three_records/w3", 3, K3, CHAIN[:3], {"n_rec=world", "non-symmetric"}, set(), set(), set(), [2, 2, 2], 0),
        C("four_records/w3", 3, K3, CHAIN, {"n_rec=world+1", "non-symmetric"}, set(), set(), set(), [2, 2, 2], 0),
        C("three_records/w2", 2, K3, CHAIN[:3], {"n_rec=world+1", "non-symmetric"}, set(), set(), set(), [2, 1], 0),
        # -- read ownership
        C("no_reads/w3", 3, [], [], {"n_reads=0", "n_rec=0"}, {0, 1, 2}, {0, 1, 2}, {0, 1, 2}, [0, 0, 0], 0),
        C("one_read/w3", 3, [1000], SELF, {"n_reads=1", "n_reads<world", "n_rec=world+1", "all records on one read", "record 0 a self-overlap, no copy"},
          {1, 2}, set(), {1, 2}, [3, 0, 0], 0),
        C("one_read_with_a_copy/w3", 3, [1000], SELF[:2] + SELF[:1] + SELF[3:], {"n_reads=1", "all records on one read", "record 0 a self-overlap, copied"},
          {1, 2}, set(), {1, 2}, [3, 0, 0], 1),
        C("long_middle_read/w4", 4, [50, 100000, 50], all_vs_all([50, 100000, 50]), {"one read holds the windows", "n_reads<world", "symmetric sorted"},
          {1, 2}, set(), {1, 2}, [3, 0, 0, 1], 1),
        C("all_lengths_zero/w3", 3, [0, 0, 0, 0], [], {"all lengths 0", "n_rec=0"}, {0, 1}, {0, 1, 2}, {0, 1, 2}, [0, 0, 0], 0),
        C("zero_lengths_on_the_bound/w2", 2, [1000, 0, 0, 1000], [(0, 100, 600, 3, 200, 700), (3, 200, 700, 0, 100, 600)],
          {"zero-length reads on a bound", "n_rec=world", "mirror last of the last rank"}, set(), set(), set(), [1, 1], 1),
        # -- stream shapes
        C("all_vs_all_16/w8", 8, K16, all_vs_all(K16), {"symmetric sorted"}, set(), set(), set(), [1] * 8, 1),
        C("all_vs_all_16/w64", 64, K16, all_vs_all(K16), {"symmetric sorted", "n_reads<world"},
          {g for g in range(64) if g % 4}, set(), {g for g in range(64) if g % 4}, [0 if g % 4 else 4 for g in range(64)], 1),
        C("all_vs_all_6/w1", 1, [1000] * 6, all_vs_all([1000] * 6), {"symmetric sorted"}, set(), set(), set(), [1], 1),
        C("all_vs_all_12_shuffled/w3", 3, [1000] * 12, shuffled(all_vs_all([1000] * 12), 53), {"symmetric shuffled"}, set(), set(), set(), [3, 3, 3], 1),
        C("half_pairs_12_shuffled/w3", 3, [1000] * 12, shuffled(all_vs_all([1000] * 12, half=True), 35), {"non-symmetric"}, set(), set(), set(), [3, 3, 3], 0),
        C("one_busy_read/w8", 8, [1000] * 8, [(5, 10 * i, 10 * i + 500, 5, 10 * i + 100, 10 * i + 600) for i in range(20)],
          {"all records on one read", "owner receives nothing"}, set(), set(), set(range(8)) - {5}, [8 if g == 5 else 0 for g in range(8)], 0),
        # -- encodings
        C("deep_windows/w4", 4, [2000] * 4, DEEP, {"width 1, exceptions past rank 0", "width 2, windows above 255 past rank 0", "owner receives nothing"},
          set(), set(), {0, 2}, [0, 3, 0, 2], 1, p=P_SHORT, widths=(1, 2)),
        C("width_8_refused/w2", 2, K3, CHAIN, {"width 8"}, set(), set(), set(), [2, 2], 0, widths=(8,)),
    ]
    for k in range(6):
        runs, nothing = {0: ([2, 1, 1], set()), 3: ([1, 2, 1], set())}.get(k, ([2, 2, 0], {2}))
        cases.append(C(f"near_mirror_{FIELDS[k]}/w3", 3, K3, [A_B, NEAR[k]],
                       {f"near mirror, {FIELDS[k]} differs", "n_rec=world-1", "n_rec<world, no mirror/w3", "non-symmetric"}, set(), {0}, nothing, runs, 0))
    return cases


CASES = _build()

CLASSES = (["n_rec=0", "n_rec=1", "n_rec=world-1", "n_rec=world", "n_rec=world+1"]
           + [f"n_rec<world, {m}/w{w}" for m in ("mirror in a later slice", "no mirror") for w in (3, 8)]
           + ["n_reads=0", "n_reads=1", "n_reads<world", "one read holds the windows", "all lengths 0", "zero-length reads on a bound", "owner receives nothing"]
           + ["record 0 a self-overlap, no copy", "record 0 a self-overlap, copied", "mirror last of the last rank"]
           + [f"near mirror, {f} differs" for f in FIELDS]
           + ["symmetric sorted", "symmetric shuffled", "non-symmetric", "all records on one read"]
           + [f"world={w}" for w in (1, 2, 3, 8, 64)]
           + ["width 1, exceptions past rank 0", "width 2, windows above 255 past rank 0", "width 8"])


def case_id(case):
    return case.name


def by_name(name):
    return next(c for c in CASES if c.name == name)


def holds(cls: str, case: PresplitCase, m: Model) -> bool:
    """Does the case fill the class, by the model?"""
    w, n, recs = case.world, case.n_rec, case.recs
    if cls.startswith("n_rec="):
        return n == {"0": 0, "1": 1, "world-1": w - 1, "world": w, "world+1": w + 1}[cls[6:]]
    if cls.startswith("n_rec<world, "):
        kind, ww = cls[13:].split("/w")
        if not (0 < n < w == int(ww) and 0 in m.empty_slices):
            return False
        return (m.symmetric and m.mirror_slice > m.first_slice) if kind == "mirror in a later slice" else not m.symmetric
    if cls.startswith("world="):
        return w == int(cls[6:])
    if cls.startswith("near mirror, "):
        k = FIELDS.index(cls.split()[2])
        want = mirror(recs[0])
        return n >= 2 and not m.symmetric and [j for j in range(6) if recs[1][j] != want[j]] == [k]
    lens = [int(x) for x in case.read_len]
    windows = [b - a for a, b in zip(m.prefix, m.prefix[1:])]
    cov = case.oracle()["cov"]
    first_rank_window = m.prefix[m.bounds[1]] if w > 1 else len(cov)
    deep = np.flatnonzero(cov >= 255)
    deep_ranks = {max(g for g in range(w) if m.prefix[m.bounds[g]] <= int(i)) for i in deep}
    return {
        "n_reads=0": lambda: len(lens) == 0,
        "n_reads=1": lambda: len(lens) == 1,
        "n_reads<world": lambda: 0 < len(lens) < w,
        "one read holds the windows": lambda: max(windows) * 10 > 9 * sum(windows) and any(0 < g < w - 1 for g in m.no_reads),
        "all lengths 0": lambda: len(lens) > 0 and not any(lens) and m.no_reads == set(range(w - 1)),
        # the tie of lower_bound: the prefix sum a bound looks for is reached by a read that zero-length reads follow
        "zero-length reads on a bound": lambda: any(m.prefix.count(m.prefix[-1] * g // w) > 1 and m.prefix[-1] * g // w > 0 for g in range(1, w)),
        "owner receives nothing": lambda: bool(m.receives_nothing - m.no_reads),
        "record 0 a self-overlap, no copy": lambda: recs[0] == mirror(recs[0]) and not m.symmetric and n > 1,
        "record 0 a self-overlap, copied": lambda: recs[0] == mirror(recs[0]) and m.symmetric,
        "mirror last of the last rank": lambda: m.symmetric and m.mirror_index == n - 1 and m.mirror_slice == w - 1 and w > 1,
        "symmetric sorted": lambda: m.symmetric and all(a[0] <= b[0] for a, b in zip(recs, recs[1:])) and len({r[0] for r in recs}) > 2,
        "symmetric shuffled": lambda: m.symmetric and any(a[0] > b[0] for a, b in zip(recs, recs[1:])),
        "non-symmetric": lambda: not m.symmetric and any(r[0] != r[3] for r in recs),
        "all records on one read": lambda: n > 1 and len({r[0] for r in recs} | {r[3] for r in recs}) == 1,
        "width 1, exceptions past rank 0": lambda: 1 in case.widths and len(deep) > 0 and int(deep[0]) >= first_rank_window and len(deep_ranks) >= 2,
        "width 2, windows above 255 past rank 0": lambda: 2 in case.widths and len(deep) > 0 and int(deep[0]) >= first_rank_window and len(deep_ranks) >= 2,
        "width 8": lambda: case.widths == (8,),
    }[cls]()
