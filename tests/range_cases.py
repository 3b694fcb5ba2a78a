"""Sets laid on the boundaries at which the ranges of the pileup kernel's hand-out begin (raft_amd/csrc/quantum.hpp Quantum).

A worker of pileup_wave_kernel draws ranges of reads; range k begins with the first read that begins at or behind window at(k).  The
sets here put reads, records and runs of high windows ON those boundaries: a read beginning on at(k) - 1, at(k) and at(k) + 1, a
read of one window and one of no window on at(k), a read ending on at(k) - 1 and on at(k), a run of high windows one window short
of repeat_length and exactly long enough across at(k) -- for every KIND of boundary the quantum has -- and long reads that leave
whole ranges without a read of their own.

    ranges_graded(B)          laid on the graded quantum of ITS OWN window count B (the engine takes it under RAFT_GRADED_MIN=0)
    ranges_uniform(n_ranges)  for set_tuning(256, ...): B / 256 + 1 == n_ranges, the placements at the first and the last range of
                              every hand-out counter's share (counter c deals out [c*q + min(c, r), ...), q, r = n_ranges divmod 8)

graded_geometry / graded_at restate the quantum in Python FORWARDS (share s begins at s * share, n_long ranges of q_long, then ranges
of q_short); tests/test_quantum.py compares them, for every B used here, with what tests/quantum_check.cpp prints from the header,
and checks that ten wrong variants of the restatement (AT_VARIANTS) are each caught.  The constants are read back from the sources in
tests/test_range_cases.py, which also pins every set to the oracle and counts, on the oracle's side, the reads of every class
(range_census).  tests/test_gpu_ranges.py runs the sets through the engine.

Like the lattice sets of raft_testlib every record is a self overlap sorted by read id, so only the query side piles up; the closed
form (coverage per window, repeats) comes from the construction.
"""
import numpy as np
import raft_testlib as T
from raft_testlib import TILE_CAP, LatticeCase

ROUND = 128                               # quantum.hpp graded_quantum: a share is a multiple of this
Q1 = TILE_CAP // 128 * 128                # engine.hip quantum_for: a tile's worth
Q_LONG, Q_SHORT, FRAC_LONG = 8 * Q1, 2 * Q1, 0.9
COUNTERS = 8                              # engine.hip launch_pileup n_ctr; pileup_wave.hpp next_range
WORKERS = 256 * 4 * 4                     # wave_launch.hip wave_grid_waves: 256 CUs, four SIMDs, RAFT_WAVE_WPS waves each
GRADED_MIN_DEFAULT = 64 * WORKERS         # tiles' worth of windows from which quantum_for grades when nothing is set
UNIFORM_Q = 256                           # set_tuning(256, ...)

RESO, HIGH, RUN_M, FLANK = 10, 3, 4, 15   # windows of 10 bases; high_cov 3; repeat_length = 4 windows; flank 15 bases
RECORD_W = 65000                          # a record ends inside its read's first 65,535 windows, or there is no window record of it (hostio.pack_windows)

GRADED_BS = (100, 129, 200_000, 888_832, 888_833, 5_900_000, 7_200_000)
UNIFORM_NS = (1, 2, 7, 8, 9, 15, 17, WORKERS - 1, WORKERS, WORKERS + 1, 8 * WORKERS + 3)

KINDS = ("share", "long-long", "long-short", "short-short", "closing")
PATTERNS = ("starts", "empty", "ends-1", "ends0", "run-short", "run-long")

AT_VARIANTS = ("share not rounded to 128", "share from B // 8", "share rounded to 256", "n_long rounded, not truncated",
               "closing range dropped", "eight tenths long", "the whole share long", "short ranges first", "short ranges of one tile's worth",
               "shares begin behind a full closing range")


def graded_geometry(B, variant=None):
    """(share, n_long, per_share) of the graded quantum of a set of B windows."""
    eighth = B // 8 if variant == "share from B // 8" else (B + 7) // 8
    unit = 256 if variant == "share rounded to 256" else ROUND
    share = eighth if variant == "share not rounded to 128" else (eighth + unit - 1) // unit * unit
    frac = {"eight tenths long": 0.8, "the whole share long": 1.0}.get(variant, FRAC_LONG)
    n_long = share * frac / Q_LONG
    n_long = int(round(n_long)) if variant == "n_long rounded, not truncated" else int(n_long)
    rest = share - n_long * Q_LONG
    q_short = Q1 if variant == "short ranges of one tile's worth" else Q_SHORT
    per_share = n_long + (rest // q_short if variant == "closing range dropped" else (rest + q_short - 1) // q_short)
    return share, n_long, per_share


def graded_at(B, variant=None):
    """at(k) for k = 0 .. 8 * per_share, built forwards."""
    share, n_long, per_share = graded_geometry(B, variant)
    q_short = Q1 if variant == "short ranges of one tile's worth" else Q_SHORT
    at, begin = [], 0
    for s in range(8):
        w = begin
        for j in range(per_share):
            at.append(w)
            long_ = j >= per_share - n_long if variant == "short ranges first" else j < n_long
            w += Q_LONG if long_ else q_short
        begin = w if variant == "shares begin behind a full closing range" else (s + 1) * share
    at.append(begin)
    return np.array(at, np.int64)


def boundary_kind(B, k):
    """Which kind of boundary k (0 <= k < 8 * per_share) is, by the ranges on its two sides."""
    share, n_long, per_share = graded_geometry(B)
    j = k % per_share
    if j == 0:
        return "share"
    if j < n_long:
        return "long-long"
    if j == n_long:
        return "long-short"
    closing_short = (share - n_long * Q_LONG) % Q_SHORT != 0
    return "closing" if j == per_share - 1 and closing_short else "short-short"


def counter_shares(n_ranges):
    """[(d0, d1)] per hand-out counter: counter c deals out the ranges [d0, d1)."""
    q, r = divmod(n_ranges, COUNTERS)
    return [(c * q + min(c, r), c * q + min(c, r) + q + (1 if c < r else 0)) for c in range(COUNTERS)]


class RangeCase(LatticeCase):
    """A LatticeCase whose reads are named by the boundary they lie at: at (every boundary's window), kinds (per boundary), role (per
    read: what the layout put it there for), plan (the (kind, pattern, window) triples the layout placed)."""

    def __init__(self, name, p, cols, expect, W, role, at, kinds, plan, B, quantum):
        zero = np.zeros(W.size, np.int64)
        super().__init__(name, p, cols, expect, zero - 1, zero, W, role)
        self.at, self.kinds, self.plan, self.B, self.quantum = at, kinds, plan, B, quantum

    def idx(self, w):
        return int(np.searchsorted(self.at, w, side="right") - 1)

    def nearest(self, w):
        """(k, d): the boundary nearest to window w and w - at(k)."""
        k = self.idx(w)
        if k + 1 < self.at.size and self.at[k + 1] - w < w - self.at[k]:
            k += 1
        return k, int(w - self.at[k])

    def coordinate(self, r):
        r = int(r)
        off = self.expect["cov_offset"]
        k, d = self.nearest(int(off[r]))
        kind = self.kinds[k] if k < len(self.kinds) else "behind the last share"
        return (f"read {r} [{self.kind[r]}] windows [{int(off[r])}, {int(off[r + 1])}), begins {d:+d} from boundary k={k} "
                f"(class {kind}, at {int(self.at[k])}) of the {self.quantum} quantum, B={self.B}")


class _Layout:
    """Reads in order, each beginning where the last ended: fillers up to a boundary, then the reads of a placement."""

    def __init__(self, fill):
        self.W, self.base, self.role, self.runs = [], [], [], []          # runs: (read, s, e)
        self.cur, self.fill, self.n_fill = 0, fill, 0

    def add(self, W, role, base=1, run=None):
        if run is not None:
            self.runs.append((len(self.W),) + run)
        self.W.append(W); self.base.append(base if W > 0 else 0); self.role.append(role)
        self.cur += W

    def fill_to(self, p):
        assert p >= self.cur, (p, self.cur)
        while self.cur < p:
            self.n_fill += 1
            self.add(min(self.fill - (self.n_fill % 3) * 7, p - self.cur), "filler")

    def place(self, pattern, p, B):
        """The reads of one pattern around the boundary at window p; False: no room."""
        lead = {"starts": 1, "empty": 0, "ends-1": 10, "ends0": 10, "run-short": 10, "run-long": 10}[pattern]
        after = {"starts": 1, "empty": 1, "ends-1": 0, "ends0": 1, "run-short": 6, "run-long": 6}[pattern]
        if p - lead < self.cur or p + after > B:
            return False
        self.fill_to(p - lead)
        if pattern == "starts":
            self.add(1, "one window before the boundary")
            self.add(1, "one window on the boundary")
        elif pattern == "empty":
            self.add(0, "no window, on the boundary")
            self.add(1, "one window on the boundary, behind a read of none")
        elif pattern == "ends-1":
            self.add(10, "ends one window before the boundary")
        elif pattern == "ends0":
            self.add(11, "ends on the boundary")
        else:
            n = RUN_M - 1 if pattern == "run-short" else RUN_M
            self.add(min(30, B - (p - 10)), f"run of {n} windows across the boundary", base=HIGH - 1, run=(8, 8 + n))
        return True


def _build(name, lay, B, at, kinds, plan, quantum):
    assert lay.cur == B, (name, lay.cur, B)
    p = T._lattice_params(RESO, HIGH, RUN_M, FLANK)
    n = len(lay.W)
    W, base = np.array(lay.W, np.int64), np.array(lay.base, np.int64)
    tail = np.where(W > 0, np.array((0, 1, RESO - 1), np.int64)[np.arange(n) % 3], 0)
    rl = (W * RESO - tail).astype(np.int32)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(W, out=off[1:])
    rr = np.array([r for r, _, _ in lay.runs], np.int64)
    ws, we = (np.array([x[i] for x in lay.runs], np.int64) for i in (1, 2))
    assert np.all((0 <= ws) & (ws < we) & (we <= W[rr]))
    rs, re_ = ws * RESO + 3, np.minimum(we * RESO - 2, rl[rr])
    assert np.all(rs // RESO == ws) and np.all((re_ - 1) // RESO == we - 1)
    qid = np.concatenate([np.repeat(np.arange(n), base), rr])
    qs = np.concatenate([np.zeros(int(base.sum()), np.int64), rs])
    covered = np.minimum(W, RECORD_W)          # (the windows the whole-read records cover: all, but for the read that reaches over nine boundaries)
    qe = np.concatenate([np.repeat(np.where(W <= RECORD_W, rl, RECORD_W * RESO).astype(np.int64), base), re_])
    order = np.argsort(qid, kind="stable")
    qid, qs, qe = (x[order].astype(np.int32) for x in (qid, qs, qe))
    diff = np.zeros(B + 1, np.int64)
    np.add.at(diff, off[:-1], base)
    np.add.at(diff, off[:-1] + covered, -base)
    np.add.at(diff, off[rr] + ws, 1)
    np.add.at(diff, off[rr] + we, -1)
    cov = np.cumsum(diff[:-1]).astype(np.int32)
    rep_count = np.zeros(n, np.int64)
    rep_s, rep_e = [], []
    for r, s, e in lay.runs:                 # (one run per read at most, reads in order)
        if lay.base[r] + 1 >= HIGH and (e - s) * RESO >= p.repeat_length:
            rep_s.append(max(s * RESO - FLANK, 0)); rep_e.append(min(e * RESO + FLANK, int(rl[r])))
            rep_count[r] += 1
    rep_offset = np.zeros(n + 1, np.int64)
    np.cumsum(rep_count, out=rep_offset[1:])
    expect = {"cov_offset": off, "cov": cov, "rep_offset": rep_offset, "rep_s": np.array(rep_s, np.int32), "rep_e": np.array(rep_e, np.int32)}
    return RangeCase(name, p, [rl, qid, qs, qe, qid.copy(), qs.copy(), qe.copy()], expect, W, lay.role, at, kinds, plan, B, quantum)


_CACHE = {}


def ranges_graded(B):
    """The set laid on the graded quantum of B windows.  Every boundary inside the set gets one pattern, the patterns taking turns
    per kind of boundary; the set's last boundary with a read gets "starts"; where the geometry has room, one read reaches over two
    boundaries of the long part, one over nine of the short part, and one of more than TILE_CAP windows (pieces) straddles a share's
    end with a run of high windows across it."""
    if ("graded", B) in _CACHE:
        return _CACHE[("graded", B)]
    share, n_long, per_share = graded_geometry(B)
    at = graded_at(B)
    n = 8 * per_share
    kinds = [boundary_kind(B, k) for k in range(n)]
    inside = [k for k in range(n) if at[k] < B]
    k_last = inside[-1]
    # the long reads: (first boundary they reach over, boundaries reached over, where they begin, windows, role, run)
    long_reads = {}
    if n_long >= 4 and 2 * per_share <= k_last:
        k = per_share + 1
        long_reads[k + 1] = (2, int(at[k]) + 40, int(at[k + 2] - at[k]) + 10, "reaches over two boundaries of the long part", None, kinds[k + 1])
    if per_share - n_long >= 11 and 3 * per_share <= k_last:
        k = 2 * per_share + n_long + 1
        long_reads[k + 1] = (9, int(at[k]) + 40, int(at[k + 9] - at[k]) + 10, "reaches over nine boundaries of the short part", None, kinds[k + 1])
    if share > 3 * TILE_CAP and 4 * per_share <= k_last:
        k = 3 * per_share                       # (the share's first boundary; with a short closing range the one before is reached over too)
        begin = int(at[k]) - TILE_CAP + 500
        first = k - 1 if at[k - 1] > begin else k
        long_reads[first] = (k - first + 1, begin, TILE_CAP + 100, "more than a tile's windows, straddles a share's end", (TILE_CAP - 502, TILE_CAP - 502 + RUN_M), kinds[k])
    lay = _Layout(3000)
    plan, turn, skip = [], {kind: 0 for kind in KINDS}, 0
    if B <= ROUND:                              # (no boundary but the first inside the set: a read of no window begins the set)
        lay.place("empty", 0, B)
        plan.append(("share", "empty", 0))
    for k in inside[1:]:
        if skip:
            skip -= 1
            continue
        p = int(at[k])
        if k in long_reads:
            reached, begin, W, role, run, kind = long_reads[k]
            lay.fill_to(begin)
            lay.add(W, role, base=HIGH - 1 if run else 1, run=run)
            plan.append((kind, role, p))
            skip = reached - 1
            continue
        order = ["starts"] if k == k_last else [PATTERNS[(turn[kinds[k]] + i) % len(PATTERNS)] for i in range(len(PATTERNS))]
        for pattern in order:
            if lay.place(pattern, p, B):
                plan.append((kinds[k], pattern, p))
                if k == k_last:
                    plan.append(("last", pattern, p))
                else:
                    turn[kinds[k]] += 1
                break
    lay.fill_to(B)                              # (the last read pads to the chosen B)
    case = _build(f"ranges_graded({B})", lay, B, at, kinds, plan, "graded")
    _CACHE[("graded", B)] = case
    return case


def ranges_uniform(n_ranges):
    """B = 256 * (n_ranges - 1) + 100 windows for set_tuning(256, ...): the patterns take turns over the boundaries that begin the first
    and the last range of every counter's share; fillers of about half a range (of six ranges from 5000 ranges on) between them."""
    if ("uniform", n_ranges) in _CACHE:
        return _CACHE[("uniform", n_ranges)]
    B = UNIFORM_Q * (n_ranges - 1) + 100
    assert B // UNIFORM_Q + 1 == n_ranges
    at = np.arange(n_ranges + 1, dtype=np.int64) * UNIFORM_Q
    kinds = ["inner"] * n_ranges
    for c, (d0, d1) in enumerate(counter_shares(n_ranges)):
        if d1 > d0:
            kinds[d1 - 1] = f"counter {c} last"
            kinds[d0] = f"counter {c} first" if d1 - d0 > 1 else f"counter {c} first and last"
    lay = _Layout(140 if n_ranges < 5000 else 1500)
    plan, turn = [], 0
    if n_ranges == 1:
        lay.place("empty", 0, B)
        plan.append((kinds[0], "empty", 0))
    for k in range(1, n_ranges):
        if kinds[k] == "inner":
            continue
        for i in range(len(PATTERNS)):
            pattern = PATTERNS[(turn + i) % len(PATTERNS)]
            if lay.place(pattern, int(at[k]), B):
                plan.append((kinds[k], pattern, int(at[k])))
                turn += 1
                break
    lay.fill_to(B)
    case = _build(f"ranges_uniform({n_ranges})", lay, B, at, kinds, plan, "uniform")
    _CACHE[("uniform", n_ranges)] = case
    return case


def range_census(case, want):
    """Counted on the ORACLE's output and the reads' cov_offset: reads by (kind of boundary, -1 / 0 / +1), reads of one and of no
    window on a boundary, reads ending on at(k) - 1 and at(k), runs of high windows across a boundary by (kind, short / long enough),
    ranges in which no read begins by the part of the share they lie in, shares in which no read begins."""
    off = np.asarray(want["cov_offset"])
    cov = np.asarray(want["cov"])
    B = int(off[-1])
    at, kinds = case.at, case.kinds
    n = len(kinds)
    census = {}

    def count(key, by=1):
        census[key] = census.get(key, 0) + by
    inside = np.flatnonzero(at[:n] < B)
    k_last = int(inside[-1])
    W = np.diff(off)
    for d in (-1, 0, 1):
        hit = np.flatnonzero(np.isin(off[:-1] - d, at[:n]) & (off[:-1] - d >= 0))
        ks = np.searchsorted(at, off[hit] - d)
        for k in ks.tolist():
            if 0 < k < n or (k == 0 and d >= 0):
                count((kinds[k], d))
                if k == k_last:
                    count(("last", d))
    on = np.isin(off[:-1], at[:n])
    count(("read of one window", "on a boundary"), int(np.sum(on & (W == 1))))
    count(("read of no window", "on a boundary"), int(np.sum(on & (W == 0))))
    ends = off[1:][W > 0] - 1                                     # (a read's last window)
    count(("read ends", "on at(k) - 1"), int(np.sum(np.isin(ends + 1, at[1:n]))))
    count(("read ends", "on at(k)"), int(np.sum(np.isin(ends, at[1:n]))))
    # maximal runs of high windows inside a read, across a boundary
    high = np.concatenate([[0], (cov >= want["high_cov"]).astype(np.int8), [0]])
    edge = np.flatnonzero(np.diff(high))
    for s, e in zip(edge[0::2].tolist(), edge[1::2].tolist()):
        r = int(np.searchsorted(off, s, side="right") - 1)
        assert e <= off[r + 1], "a run of high windows crosses a read's end"
        k = int(np.searchsorted(at, s, side="right"))
        if k < n and s < at[k] < e:
            enough = (e - s) * case.p.reso >= case.p.repeat_length
            count((kinds[k], "run across", "long enough" if enough else "one short"))
            got = int(want["rep_offset"][r + 1] - want["rep_offset"][r])
            assert got == (1 if enough else 0), case.coordinate(r)
    # ranges in which no read begins
    begins = np.bincount(np.searchsorted(at, off[:-1], side="right") - 1, minlength=n + 1)[:n]
    if case.quantum == "graded":
        share, n_long, per_share = graded_geometry(case.B)
        for k in np.flatnonzero(begins == 0).tolist():
            if at[k] < B:
                count(("no read begins in a range", "long part" if k % per_share < n_long else "short part"))
        for s in range(8):
            if begins[s * per_share:(s + 1) * per_share].sum() == 0:
                count(("no read begins in a share",))
    else:
        count(("no read begins in a range",), int(np.sum(begins == 0)))
    return census


def census_wanted(case):
    """The classes the layout's plan must have filled, from the plan alone."""
    keys = set()
    for kind, what, p in case.plan:
        if what == "starts":
            keys |= {(kind, -1), (kind, 0), ("read of one window", "on a boundary")} | ({(kind, 1)} if p + 1 < case.B else set())
        elif what == "empty":
            keys |= {(kind, 0), ("read of no window", "on a boundary"), ("read of one window", "on a boundary")}
        elif what == "ends-1":
            keys |= {(kind, 0), ("read ends", "on at(k) - 1")}
        elif what == "ends0":
            keys |= {("read ends", "on at(k)")} | ({(kind, 1)} if p + 1 < case.B else set())
        elif what in ("run-short", "run-long") and kind != "last":
            keys.add((kind, "run across", "one short" if what == "run-short" else "long enough"))
        elif what.startswith("reaches over two"):
            keys.add(("no read begins in a range", "long part"))
        elif what.startswith("reaches over nine"):
            keys.add(("no read begins in a range", "short part"))
        elif what.startswith("more than a tile"):
            keys.add((kind, "run across", "long enough"))
    return sorted(keys, key=str)


def three_runs(case):
    """(qid, qs, qe) of the set as three runs sorted by read id, one behind the other (what a mirrored stream looks like to the engine:
    tile_desc_kernel searches every boundary in every run): record i of read r goes to run (r + i) % 3."""
    qid, qs, qe = case.cols[1:4]
    first = np.searchsorted(qid, qid, side="left")
    run = (qid + (np.arange(qid.size) - first)) % 3
    order = np.argsort(run, kind="stable")
    return qid[order], qs[order], qe[order]
