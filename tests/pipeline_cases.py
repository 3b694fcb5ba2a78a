"""The sets that put the chunked host pipeline (raft_amd/csrc/engine_pipeline.hip: raft_hip_run_pipelined, raft_hip_run_multi, _grouped,
_windows and the host-routed path) on its structural edges, and a plain-Python model of its arithmetic: the chunk plan with the delta4
boundary moves, where every context's outputs start, the routed path's bounds.

A case is tiny: a few reads, a few dozen records in one to five sorted runs, a number of chunks.  What it is FOR is written beside it
twice: the classes it claims to fill (CLASSES: the census of tests/test_pipeline_cases.py fails on an empty one) and what the planner
makes of it -- per chunk (r0, r1, records per run, win_lo), per number of contexts and job (first_chunk, n_chunks, bins0, rep_room,
frag_room), or "one piece" / "routed" / "redo".  Both are literals here; tests/test_pipeline_cases.py holds them against the model below and
against the real planner (tests/pipeline_plan_print.cpp over pipeline_plan.hpp), so a case that stops reaching its edge fails on the CPU
instead of quietly testing something else on the GPU.

Nothing here needs a device."""
from __future__ import annotations

from bisect import bisect_left

import numpy as np
from presplit_cases import P_SHORT
from raft_testlib import RaftParams, oracle_run

RESO = P_SHORT.reso
MINBINS = max((P_SHORT.repeat_length + RESO - 1) // RESO, 1)       # two windows at or above high_cov are a repeat
SAMPLES = 8192                                                     # what the planner looks at before it believes in sorted runs
MAX_SEG = 4                                                        # sorted runs a chunk plan keeps pieces for
D4_BLOCK = 1024                                                    # windows per anchor of the four-bit step encoding
CONTEXTS = (1, 2, 3)


def sym(p):
    return RaftParams(**dict(p.__dict__, symmetric_mode=1))


def n_win(ln, reso=RESO):
    return (int(ln) + reso - 1) // reso if ln > 0 else 0


def window_prefix(read_len, reso=RESO):
    w = [0]
    for ln in read_len:
        w.append(w[-1] + n_win(ln, reso))
    return w


# ---- the model: the planner's arithmetic, restated ------------------------------------------------------------------------------

def sampled_runs(qid):
    """Where the planner believes the sorted runs of a query column begin: it compares min(n, 8192) evenly spread samples with their
    predecessors and bisects between two that descend.  None: more than four runs."""
    n = len(qid)
    s = min(n, SAMPLES)
    start, prev = [0], 0
    for i in range(1, s):
        pos = i * (n - 1) // (s - 1)
        if qid[pos] < qid[prev]:
            lo, hi = prev, pos
            while hi - lo > 1:
                mid = (lo + hi) // 2
                if qid[mid] >= qid[prev]:
                    lo = mid
                else:
                    hi = mid
            if len(start) == MAX_SEG:
                return None
            start.append(hi)
        prev = pos
    return start + [n]


def model_plan(read_len, run_ids, n_chunks, d4, reso=RESO, events=None):
    """Chunks [(r0, r1, (records per run), win_lo)] of a job: read boundaries that balance the records -- boundary k is the first read
    with n_rec k / want records before it, kept when it lies after the one before and before the end -- and for delta4 every inner
    boundary moved forward to the next read that begins on a multiple of 4 windows, dropped when an earlier one has passed it or no such
    read exists.  run_ids: the query ids of every sorted run.  events: takes (boundary, moved to | None, why) per boundary (delta4)."""
    n_reads, n_rec = len(read_len), sum(len(r) for r in run_ids)
    want = min(n_chunks, n_reads)
    below = lambda r: sum(bisect_left(run, r) for run in run_ids)
    bound = [0]
    for k in range(1, want):
        target = n_rec * k // want
        r = next(r for r in range(bound[-1], n_reads + 1) if below(r) >= target)
        if bound[-1] < r < n_reads:
            bound.append(r)
    W = window_prefix(read_len, reso)
    if d4:
        moved = [0]
        for b in bound[1:]:
            if b <= moved[-1]:
                if events is not None:
                    events.append((b, None, "passed"))
                continue
            r = b
            while W[r] % 4 and r < n_reads:
                r += 1
            if r < n_reads and W[r] % 4 == 0:
                moved.append(r)
            if events is not None:
                events.append((b, r if r < n_reads else None, "moved" if r < n_reads else "ran out"))
        bound = moved
    bound.append(n_reads)
    return [(a, b, tuple(bisect_left(run, b) - bisect_left(run, a) for run in run_ids), W[a] if d4 else 0) for a, b in zip(bound, bound[1:])]


def model_jobs(plan, n_ctx, read_len, p=P_SHORT):
    """[(first_chunk, n_chunks, bins0, rep_room, frag_room)] per context that takes part, and what the caller's arrays must hold
    (bins, repeats, fragments): consecutive chunks each; a job's windows are exact, its repeats and fragments start at the sums of the
    bounds of the jobs before it.  One context: no rooms (the caller's capacities are the limits)."""
    n_ch, n_job = len(plan), min(n_ctx, len(plan))
    minbins = max((p.repeat_length + p.reso - 1) // p.reso, 1)
    jobs, bins, rep, frag = [], 0, 0, 0
    for d in range(n_job):
        first, end = n_ch * d // n_job, n_ch * (d + 1) // n_job
        if n_job == 1:
            return [(first, end - first, 0, 0, 0)], (0, 0, 0)
        reads = range(plan[first][0], plan[end - 1][1])
        jb, jl = sum(n_win(read_len[r], p.reso) for r in reads), sum(int(read_len[r]) for r in reads)
        rep_room, frag_room = (jb + len(reads)) // (minbins + 1), jl // p.interval_length + 2 * len(reads)
        jobs.append((first, end - first, bins, rep_room, frag_room))
        bins, rep, frag = bins + jb, rep + rep_room, frag + frag_room
    return jobs, (bins, rep, frag)


def routed_sides(n_reads, recs6, symmetric):
    """Intervals per read of the host-routed path: query sides, and target sides on another read unless the stream is symmetric."""
    cnt = [0] * n_reads
    for q, _, _, t, _, _ in recs6:
        cnt[q] += 1
        if not symmetric and t != q:
            cnt[t] += 1
    return cnt


def model_routed(n_reads, recs6, symmetric, n_chunks, n_ctx):
    """Read bounds of the host-routed path's chunks: max(n_chunks, n_ctx) of them at most, no more than there are reads; bound k is the
    first read with total k / want intervals before it, kept like the plan's."""
    pre = [0]
    for c in routed_sides(n_reads, recs6, symmetric):
        pre.append(pre[-1] + c)
    want = max(1, min(max(n_chunks, n_ctx), max(n_reads, 1)))
    bound = [0]
    for k in range(1, want):
        r = bisect_left(pre, pre[-1] * k // want)
        if bound[-1] < r < n_reads:
            bound.append(r)
    return bound + [n_reads]


# ---- a case ---------------------------------------------------------------------------------------------------------------------

class PipeCase:
    """runs: the records (qid, qs, qe) of every sorted run.  route: "chunked", "one piece" (the plan has one chunk, or the engine takes no
    plan), "routed" (plain columns that are no handful of runs) or "redo" (a plan the chunks' own checks refute: the job again in one
    piece).  plan / jobs: the literal claims for the byte encodings, plan8 / jobs8 for delta4 (widths holds 8)."""

    def __init__(self, name, read_len, runs, n_chunks, classes, plan, jobs=None, plan8=None, jobs8=None, route="chunked", widths=(1,),
                 forms=("derived", "columns", "grouped", "windows"), p=P_SHORT):
        self.name, self.n_chunks, self.route, self.widths, self.forms, self.p = name, n_chunks, route, tuple(widths), tuple(forms), sym(p)
        self.read_len = np.asarray(read_len, np.int32).reshape(-1)
        self.runs = [[tuple(int(x) for x in r) for r in run] for run in runs]
        self.classes = frozenset(classes)
        self.plan, self.jobs, self.plan8, self.jobs8 = plan, jobs or {}, plan8, jobs8 or {}
        self._want = None

    n_reads = property(lambda self: len(self.read_len))
    n_rec = property(lambda self: sum(len(r) for r in self.runs))
    n_runs = property(lambda self: len(self.runs))
    run_ids = property(lambda self: [[r[0] for r in run] for run in self.runs])

    @property
    def cols(self):
        """qid, qs, qe of the stream: the runs one after the other."""
        a = np.asarray([r for run in self.runs for r in run], np.int32).reshape(-1, 3)
        return [np.ascontiguousarray(a[:, k]) for k in range(3)]

    @property
    def offsets(self):
        """The grouped form: int64 [n_runs, n_reads + 1], first record of every read in every run."""
        off, at = np.zeros((self.n_runs, self.n_reads + 1), np.int64), 0
        for g, ids in enumerate(self.run_ids):
            off[g] = at + np.searchsorted(np.asarray(ids, np.int64), np.arange(self.n_reads + 1))
            at += len(ids)
        return off

    @property
    def descents(self):
        """Sorted runs of the stream as it is: one more than the places where the query id steps back."""
        q = self.cols[0]
        return 1 + int(np.count_nonzero(np.diff(q) < 0))

    def plan_for(self, width):
        """The claimed plan in this width: None when the job goes through in one piece."""
        if self.route != "chunked":
            return None
        plan = self.plan8 if width == 8 else self.plan
        return plan if plan is not None and len(plan) >= 2 else None

    def oracle(self):
        """The oracle's outputs for the whole set (computed once, never written to)."""
        if self._want is None:
            q, s, e = self.cols
            self._want = oracle_run(self.p, self.read_len, q, s, e, q, s, e)
            self._want["symmetric"] = 1                    # (asserted by the caller: every record is its own target side here)
            for v in self._want.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        return self._want

    def __repr__(self):
        return self.name


# ---- streams --------------------------------------------------------------------------------------------------------------------

def thin(read, n, length, salt=0):
    """n records spread over a read: no window reaches high_cov (n < 45)."""
    half = max(length // 2, 1)
    return [(read, (7 * j + 3 * salt) % half, min(length, (7 * j + 3 * salt) % half + 1 + (11 * j + salt) % half)) for j in range(n)]


def pile(read, s, e, n):
    """n copies of one interval: every window of [s, e) at depth n."""
    return [(read, s, e)] * n


def over(reads, n, length, salt=0):
    return [r for read in reads for r in thin(read, n, length, salt + read)]


def twin_piles(read, k, n=50):
    """k repeats on a read of 3 k - 1 windows: two windows at depth n, one empty, two at depth n ... -- as many as the bound of
    include/raft_hip.h allows the read, (windows + 1) / (minbins + 1)."""
    return [r for j in range(k) for r in pile(read, 150 * j, 150 * j + 100, n)]


K6 = [200] * 6                                       # four windows each
DESCENT_AT = 6003                                    # a position the planner's samples of DESCENT's 9,000 records skip


def _descent():
    """9,000 sorted records and one that steps back between two samples: the planner believes in one run."""
    recs = over(range(60), 150, 2000)
    assert len(recs) == 9000 and recs[DESCENT_AT][0] == 40
    recs[DESCENT_AT] = (2, 100, 900)
    return recs


CLAIMS = {}            # per case name: what the planner makes of it (filled below; held against the planner and the model on the CPU)


def _build():
    C = PipeCase
    k = lambda name: CLAIMS[name]
    ev = lambda reads, n, ln: [over(reads, n, ln)]
    deep6 = [[r for read in range(6) for r in pile(read, 0, 100, 260)]]
    specs = [
        # -- plan shape
        ("empty_tail/c3", K6, [thin(0, 40, 200)], 3, {"last chunk without records", "closing offsets behind an empty chunk", "no repeats"}, {}),
        ("zero_tail/c3", (2000, 0, 0, 0, 0), [thin(0, 40, 2000)], 3,
         {"chunk without records or windows", "closing offsets behind an empty chunk"}, dict(widths=(1, 8))),
        ("all_on_last/c3", K6, [thin(5, 40, 200)], 3, {"all records on the last read: one piece"}, dict(route="one piece")),
        ("one_chunk/c1", K6, ev(range(6), 5, 200), 1, {"n_chunks = 1: one piece"}, dict(route="one piece")),
        ("two_by_two/c2", [200, 200], [[(0, 10, 120), (1, 30, 200)]], 2,
         {"two reads, two records, two chunks", "chunk of one read with one record", "n_chunks = n_reads", "more contexts than chunks"}, {}),
        ("two_by_two/c3", [200, 200], [[(0, 10, 120), (1, 30, 200)]], 3, {"n_chunks above n_reads"}, {}),
        ("two_by_two/c50", [200, 200], [[(0, 10, 120), (1, 30, 200)]], 50, {"n_chunks far above n_reads"}, dict(widths=(1, 2, 8))),
        ("five/c5", [200] * 5, ev(range(5), 3, 200), 5, {"5 chunks on one context", "jobs of unequal chunk counts"}, {}),
        ("eight/c8", [200] * 8, ev(range(8), 3, 200), 8,
         {"8 chunks on one context", "jobs of unequal chunk counts", "delta4: several chunks inside one anchor block",
          "delta4: a chunk inside a block another context's chunk began"}, dict(widths=(1, 8))),
        ("nine/c9", [150] * 9, ev(range(9), 3, 150), 9,
         {"9 chunks on one context", "n_chunks = n_reads", "delta4: boundary moved by three reads", "delta4: boundary dropped, an earlier one passed it",
          "delta4: odd window count"}, dict(widths=(1, 2, 8))),
        ("seven/c7", [150] * 7, ev(range(7), 3, 150), 7, {"delta4: boundary dropped, the move ran to n_reads", "delta4: odd window count"}, dict(widths=(1, 8))),
        ("moves/c11", [50 * w for w in (2, 2, 2, 1, 1, 4, 1, 1, 1, 1, 4)], ev(range(11), 3, 50), 11,
         {"delta4: boundary moved by one read", "delta4: boundary moved by two reads", "delta4: boundary moved by three reads",
          "delta4: boundary dropped, an earlier one passed it"}, dict(widths=(1, 8))),
        # -- runs
        ("two_runs/c3", [200] * 5, [[(q, 10 + i, 150 + i) for i, q in enumerate((0, 0, 0, 1, 4, 4, 4))], [(q, 20 + i, 90 + 9 * i) for i, q in enumerate((2, 2, 2))]], 3,
         {"runs: 2", "run absent from the first chunk", "run absent from the last chunk"}, {}),
        ("three_runs/c3", K6, [over(range(6), 2, 200), over((1, 2), 3, 200, 5), pile(1, 20, 180, 7)], 3,
         {"runs: 3", "run inside one read", "run absent from the last chunk"}, {}),
        ("four_runs/c3", K6, [over(range(6), 2, 200), over((1, 2), 3, 200, 5), pile(1, 20, 180, 7), over((0, 5), 4, 200, 9)], 3,
         {"runs: 4", "run absent from a middle chunk"}, dict(widths=(1, 8))),
        ("empty_run/c3", K6, [over(range(6), 3, 200), [], over((2, 3), 2, 200, 4)], 3, {"runs: 3", "grouped run without records"},
         dict(forms=("grouped", "windows"))),
        ("five_plain/c3", K6, [over(range(6), 2, 200, g) for g in range(5)], 3, {"five plain runs: routed", "five plain runs, delta4: one piece"},
         dict(route="routed", forms=("derived", "columns"), widths=(1, 8))),
        ("five_grouped/c3", K6, [over(range(6), 2, 200, g) for g in range(5)], 3, {"five grouped runs: one piece"},
         dict(route="one piece", forms=("grouped", "windows"))),
        ("gaps/c3", [150] * 12, ev((0, 1, 6, 7), 6, 150), 3,
         {"runs: 1", "reads without records at a chunk's first position", "reads without records at a chunk's last position",
          "reads without records on both sides of a boundary"}, dict(widths=(1, 8))),
        ("zeros_between/c4", [0, 200, 0, 0, 200, 0, 200, 0], ev((1, 4, 6), 8, 200), 4,
         {"runs: 1", "reads without windows at a chunk's ends", "reads without records at a chunk's first position"}, dict(widths=(1, 2, 8))),
        ("descent/c4", [2000] * 60, [_descent()], 4, {"a descent between two samples"}, dict(route="redo", forms=("derived", "columns"))),
        # -- stitching
        ("reps_first/c2", [250] * 4, [twin_piles(0, 2) + over((1, 2, 3), 30, 250)], 2,
         {"repeats only in the first job", "a job's repeats equal its room", "close_gaps moves nothing"}, {}),
        ("reps_last/c2", [250] * 4, [over((0, 1, 2), 40, 250) + twin_piles(3, 2)], 2,
         {"repeats only in the last job", "close_gaps moves over a gap of its full room", "the last job is one read", "a job's repeats equal its room"}, {}),
        ("reps_every/c4", [250] * 4, [[r for read in range(4) for r in twin_piles(read, 2)]], 4,
         {"repeats in every job", "a job's repeats equal its room", "close_gaps moves nothing"}, {}),
        ("reps_mixed/c4", [250] * 4, [pile(0, 0, 100, 100) + [r for read in (1, 2, 3) for r in twin_piles(read, 2)]], 4,
         {"repeats in every job", "close_gaps moves real data", "fragments in every job"}, dict(widths=(1, 2))),
        ("exc_every/c6", K6, deep6, 6, {"exceptions in every job", "fragments in every job"}, dict(widths=(1, 2, 8))),
        ("exc_last/c3", K6, [over(range(5), 30, 200) + pile(5, 0, 100, 260)], 3, {"exceptions only in the last chunk", "the last job is one read"}, {}),
        # -- delta4 and the anchors' blocks
        ("blocks/c16", [12800] * 16, ev(range(16), 3, 12800), 16,
         {"delta4: a chunk begins exactly on a block", "delta4: a chunk ends exactly on a block", "delta4: a chunk inside a block another context's chunk began",
          "delta4: several chunks inside one anchor block", "no exceptions"}, dict(widths=(1, 8))),
        ("blocks_askew/c8", [12850] * 8, ev(range(8), 3, 12850), 8, {"delta4: a chunk begins inside a block", "delta4: boundary moved by three reads"}, dict(widths=(8,))),
    ]
    return [C(name, lens, runs, n_chunks, classes, **dict(kw, **CLAIMS.get(name, dict(plan=None)))) for name, lens, runs, n_chunks, classes, kw in specs]


class RoutedCase:
    """Six-column records that are no handful of sorted runs, or whose flag is not asserted: the host-routed path.  bounds: the claimed
    read bounds of its chunks per number of contexts."""

    def __init__(self, name, read_len, recs, mode, n_chunks, classes, bounds):
        self.name, self.mode, self.n_chunks, self.classes, self.bounds = name, mode, n_chunks, frozenset(classes), bounds
        self.read_len = np.asarray(read_len, np.int32)
        self.recs = [tuple(int(x) for x in r) for r in recs]
        self.p = RaftParams(**dict(P_SHORT.__dict__, symmetric_mode=mode))
        self._want = None

    n_reads = property(lambda self: len(self.read_len))

    @property
    def cols(self):
        a = np.asarray(self.recs, np.int32).reshape(-1, 6)
        return [np.ascontiguousarray(a[:, k]) for k in range(6)]

    def oracle(self, p=None):
        if p is not None:
            return oracle_run(p, self.read_len, *self.cols)
        if self._want is None:
            self._want = oracle_run(self.p, self.read_len, *self.cols)
        return self._want

    def __repr__(self):
        return self.name


def _routed():
    R = RoutedCase
    ids = [(5 * i + 1) % 8 for i in range(40)]
    mixed = [((1, 2, 5, 6)[q % 4], 5 + i, 100 + 2 * i, (6, 5, 2, 1)[(q + i) % 4], 30 + i, 150 + i) for i, q in enumerate(ids)]
    return [
        R("routed_one_read/c9", [200] * 4, [(2, 3 * i, 100 + 3 * i, 2, 3 * i, 100 + 3 * i) for i in range(30)], 0, 9,
          {"routed: n_chunks above n_reads", "routed: every interval on one read", "routed: records with tid == qid", "routed: more contexts than chunks"},
          {1: [0, 3, 4], 2: [0, 3, 4], 3: [0, 3, 4]}),
        R("routed_mixed/c3", [200] * 8, mixed, -1, 3, {"routed: reads without intervals at a chunk's ends"},
          {1: [0, 3, 6, 8], 2: [0, 3, 6, 8], 3: [0, 3, 6, 8]}),
        R("routed_mixed/c8", [200] * 8, mixed + [(5, 0, 50, 5, 100, 150)], 0, 8,
          {"routed: a chunk of one read", "routed: records with tid == qid", "routed: reads without intervals at a chunk's ends"},
          {1: [0, 2, 3, 6, 7, 8], 2: [0, 2, 3, 6, 7, 8], 3: [0, 2, 3, 6, 7, 8]}),
    ]


# what the planner makes of every case: (r0, r1, records per run, win_lo) per chunk; per number of contexts ((first_chunk, n_chunks, bins0,
# rep_room, frag_room) per job, (bins, repeats, fragments) the caller's arrays must hold); plan8 / jobs8: the same for delta4
CLAIMS.update({
    'empty_tail/c3': dict(
        plan=[(0, 1, (40,), 0), (1, 6, (0,), 0)],
        jobs={2: ([(0, 1, 0, 1, 4), (1, 1, 4, 8, 20)], (24, 9, 24)), 3: ([(0, 1, 0, 1, 4), (1, 1, 4, 8, 20)], (24, 9, 24))},
    ),
    'zero_tail/c3': dict(
        plan=[(0, 1, (40,), 0), (1, 5, (0,), 0)],
        jobs={2: ([(0, 1, 0, 13, 22), (1, 1, 40, 1, 8)], (40, 14, 30)), 3: ([(0, 1, 0, 13, 22), (1, 1, 40, 1, 8)], (40, 14, 30))},
        plan8=[(0, 1, (40,), 0), (1, 5, (0,), 40)],
        jobs8={2: ([(0, 1, 0, 13, 22), (1, 1, 40, 1, 8)], (40, 14, 30)), 3: ([(0, 1, 0, 13, 22), (1, 1, 40, 1, 8)], (40, 14, 30))},
    ),
    'all_on_last/c3': dict(
        plan=[(0, 6, (40,), 0)],
        jobs={2: ([(0, 1, 0, 0, 0)], (0, 0, 0)), 3: ([(0, 1, 0, 0, 0)], (0, 0, 0))},
    ),
    'one_chunk/c1': dict(
        plan=[(0, 6, (30,), 0)],
        jobs={2: ([(0, 1, 0, 0, 0)], (0, 0, 0)), 3: ([(0, 1, 0, 0, 0)], (0, 0, 0))},
    ),
    'two_by_two/c2': dict(
        plan=[(0, 1, (1,), 0), (1, 2, (1,), 0)],
        jobs={2: ([(0, 1, 0, 1, 4), (1, 1, 4, 1, 4)], (8, 2, 8)), 3: ([(0, 1, 0, 1, 4), (1, 1, 4, 1, 4)], (8, 2, 8))},
    ),
    'two_by_two/c3': dict(
        plan=[(0, 1, (1,), 0), (1, 2, (1,), 0)],
        jobs={2: ([(0, 1, 0, 1, 4), (1, 1, 4, 1, 4)], (8, 2, 8)), 3: ([(0, 1, 0, 1, 4), (1, 1, 4, 1, 4)], (8, 2, 8))},
    ),
    'two_by_two/c50': dict(
        plan=[(0, 1, (1,), 0), (1, 2, (1,), 0)],
        jobs={2: ([(0, 1, 0, 1, 4), (1, 1, 4, 1, 4)], (8, 2, 8)), 3: ([(0, 1, 0, 1, 4), (1, 1, 4, 1, 4)], (8, 2, 8))},
        plan8=[(0, 1, (1,), 0), (1, 2, (1,), 4)],
        jobs8={2: ([(0, 1, 0, 1, 4), (1, 1, 4, 1, 4)], (8, 2, 8)), 3: ([(0, 1, 0, 1, 4), (1, 1, 4, 1, 4)], (8, 2, 8))},
    ),
    'five/c5': dict(
        plan=[(0, 1, (3,), 0), (1, 2, (3,), 0), (2, 3, (3,), 0), (3, 4, (3,), 0), (4, 5, (3,), 0)],
        jobs={2: ([(0, 2, 0, 3, 8), (2, 3, 8, 5, 12)], (20, 8, 20)), 3: ([(0, 1, 0, 1, 4), (1, 2, 4, 3, 8), (3, 2, 12, 3, 8)], (20, 7, 20))},
    ),
    'eight/c8': dict(
        plan=[(0, 1, (3,), 0), (1, 2, (3,), 0), (2, 3, (3,), 0), (3, 4, (3,), 0), (4, 5, (3,), 0), (5, 6, (3,), 0), (6, 7, (3,), 0), (7, 8, (3,), 0)],
        jobs={2: ([(0, 4, 0, 6, 16), (4, 4, 16, 6, 16)], (32, 12, 32)), 3: ([(0, 2, 0, 3, 8), (2, 3, 8, 5, 12), (5, 3, 20, 5, 12)], (32, 13, 32))},
        plan8=[(0, 1, (3,), 0), (1, 2, (3,), 4), (2, 3, (3,), 8), (3, 4, (3,), 12), (4, 5, (3,), 16), (5, 6, (3,), 20), (6, 7, (3,), 24), (7, 8, (3,), 28)],
        jobs8={2: ([(0, 4, 0, 6, 16), (4, 4, 16, 6, 16)], (32, 12, 32)), 3: ([(0, 2, 0, 3, 8), (2, 3, 8, 5, 12), (5, 3, 20, 5, 12)], (32, 13, 32))},
    ),
    'nine/c9': dict(
        plan=[(0, 1, (3,), 0), (1, 2, (3,), 0), (2, 3, (3,), 0), (3, 4, (3,), 0), (4, 5, (3,), 0), (5, 6, (3,), 0), (6, 7, (3,), 0), (7, 8, (3,), 0), (8, 9, (3,), 0)],
        jobs={2: ([(0, 4, 0, 5, 14), (4, 5, 12, 6, 17)], (27, 11, 31)), 3: ([(0, 3, 0, 4, 10), (3, 3, 9, 4, 10), (6, 3, 18, 4, 10)], (27, 12, 30))},
        plan8=[(0, 4, (12,), 0), (4, 8, (12,), 12), (8, 9, (3,), 24)],
        jobs8={2: ([(0, 1, 0, 5, 14), (1, 2, 12, 6, 17)], (27, 11, 31)), 3: ([(0, 1, 0, 5, 14), (1, 1, 12, 5, 14), (2, 1, 24, 1, 3)], (27, 11, 31))},
    ),
    'seven/c7': dict(
        plan=[(0, 1, (3,), 0), (1, 2, (3,), 0), (2, 3, (3,), 0), (3, 4, (3,), 0), (4, 5, (3,), 0), (5, 6, (3,), 0), (6, 7, (3,), 0)],
        jobs={2: ([(0, 3, 0, 4, 10), (3, 4, 9, 5, 14)], (21, 9, 24)), 3: ([(0, 2, 0, 2, 7), (2, 2, 6, 2, 7), (4, 3, 12, 4, 10)], (21, 8, 24))},
        plan8=[(0, 4, (12,), 0), (4, 7, (9,), 12)],
        jobs8={2: ([(0, 1, 0, 5, 14), (1, 1, 12, 4, 10)], (21, 9, 24)), 3: ([(0, 1, 0, 5, 14), (1, 1, 12, 4, 10)], (21, 9, 24))},
    ),
    'moves/c11': dict(
        plan=[(0, 1, (3,), 0), (1, 2, (3,), 0), (2, 3, (3,), 0), (3, 4, (3,), 0), (4, 5, (3,), 0), (5, 6, (3,), 0), (6, 7, (3,), 0), (7, 8, (3,), 0), (8, 9, (3,), 0), (9, 10, (3,), 0), (10, 11, (3,), 0)],
        jobs={2: ([(0, 5, 0, 4, 14), (5, 6, 8, 6, 18)], (20, 10, 32)), 3: ([(0, 3, 0, 3, 9), (3, 4, 6, 3, 11), (7, 4, 13, 3, 11)], (20, 9, 31))},
        plan8=[(0, 2, (6,), 0), (2, 5, (9,), 4), (5, 6, (3,), 8), (6, 10, (12,), 12), (10, 11, (3,), 16)],
        jobs8={2: ([(0, 2, 0, 4, 14), (2, 3, 8, 6, 18)], (20, 10, 32)), 3: ([(0, 1, 0, 2, 6), (1, 2, 4, 4, 12), (3, 2, 12, 4, 14)], (20, 10, 32))},
    ),
    'two_runs/c3': dict(
        plan=[(0, 1, (3, 0), 0), (1, 3, (1, 3), 0), (3, 5, (3, 0), 0)],
        jobs={2: ([(0, 1, 0, 1, 4), (1, 2, 4, 6, 16)], (20, 7, 20)), 3: ([(0, 1, 0, 1, 4), (1, 1, 4, 3, 8), (2, 1, 12, 3, 8)], (20, 7, 20))},
    ),
    'three_runs/c3': dict(
        plan=[(0, 2, (4, 3, 7), 0), (2, 3, (2, 3, 0), 0), (3, 6, (6, 0, 0), 0)],
        jobs={2: ([(0, 1, 0, 3, 8), (1, 2, 8, 6, 16)], (24, 9, 24)), 3: ([(0, 1, 0, 3, 8), (1, 1, 8, 1, 4), (2, 1, 12, 5, 12)], (24, 9, 24))},
    ),
    'four_runs/c3': dict(
        plan=[(0, 2, (4, 3, 7, 4), 0), (2, 3, (2, 3, 0, 0), 0), (3, 6, (6, 0, 0, 4), 0)],
        jobs={2: ([(0, 1, 0, 3, 8), (1, 2, 8, 6, 16)], (24, 9, 24)), 3: ([(0, 1, 0, 3, 8), (1, 1, 8, 1, 4), (2, 1, 12, 5, 12)], (24, 9, 24))},
        plan8=[(0, 2, (4, 3, 7, 4), 0), (2, 3, (2, 3, 0, 0), 8), (3, 6, (6, 0, 0, 4), 12)],
        jobs8={2: ([(0, 1, 0, 3, 8), (1, 2, 8, 6, 16)], (24, 9, 24)), 3: ([(0, 1, 0, 3, 8), (1, 1, 8, 1, 4), (2, 1, 12, 5, 12)], (24, 9, 24))},
    ),
    'empty_run/c3': dict(
        plan=[(0, 3, (9, 0, 2), 0), (3, 4, (3, 0, 2), 0), (4, 6, (6, 0, 0), 0)],
        jobs={2: ([(0, 1, 0, 5, 12), (1, 2, 12, 5, 12)], (24, 10, 24)), 3: ([(0, 1, 0, 5, 12), (1, 1, 12, 1, 4), (2, 1, 16, 3, 8)], (24, 9, 24))},
    ),
    'five_plain/c3': dict(
        plan=[(0, 2, (4, 4, 4, 4, 4), 0), (2, 4, (4, 4, 4, 4, 4), 0), (4, 6, (4, 4, 4, 4, 4), 0)],
        jobs={2: ([(0, 1, 0, 3, 8), (1, 2, 8, 6, 16)], (24, 9, 24)), 3: ([(0, 1, 0, 3, 8), (1, 1, 8, 3, 8), (2, 1, 16, 3, 8)], (24, 9, 24))},
        plan8=[(0, 2, (4, 4, 4, 4, 4), 0), (2, 4, (4, 4, 4, 4, 4), 8), (4, 6, (4, 4, 4, 4, 4), 16)],
        jobs8={2: ([(0, 1, 0, 3, 8), (1, 2, 8, 6, 16)], (24, 9, 24)), 3: ([(0, 1, 0, 3, 8), (1, 1, 8, 3, 8), (2, 1, 16, 3, 8)], (24, 9, 24))},
    ),
    'five_grouped/c3': dict(
        plan=[(0, 2, (4, 4, 4, 4, 4), 0), (2, 4, (4, 4, 4, 4, 4), 0), (4, 6, (4, 4, 4, 4, 4), 0)],
        jobs={2: ([(0, 1, 0, 3, 8), (1, 2, 8, 6, 16)], (24, 9, 24)), 3: ([(0, 1, 0, 3, 8), (1, 1, 8, 3, 8), (2, 1, 16, 3, 8)], (24, 9, 24))},
    ),
    'gaps/c3': dict(
        plan=[(0, 2, (12,), 0), (2, 7, (6,), 0), (7, 12, (6,), 0)],
        jobs={2: ([(0, 1, 0, 2, 7), (1, 2, 6, 13, 35)], (36, 15, 42)), 3: ([(0, 1, 0, 2, 7), (1, 1, 6, 6, 17), (2, 1, 21, 6, 17)], (36, 14, 41))},
        plan8=[(0, 4, (12,), 0), (4, 8, (12,), 12), (8, 12, (0,), 24)],
        jobs8={2: ([(0, 1, 0, 5, 14), (1, 2, 12, 10, 28)], (36, 15, 42)), 3: ([(0, 1, 0, 5, 14), (1, 1, 12, 5, 14), (2, 1, 24, 5, 14)], (36, 15, 42))},
    ),
    'zeros_between/c4': dict(
        plan=[(0, 2, (8,), 0), (2, 5, (8,), 0), (5, 7, (8,), 0), (7, 8, (0,), 0)],
        jobs={2: ([(0, 2, 0, 4, 14), (2, 2, 8, 2, 8)], (12, 6, 22)), 3: ([(0, 1, 0, 2, 6), (1, 1, 4, 2, 8), (2, 2, 8, 2, 8)], (12, 6, 22))},
        plan8=[(0, 2, (8,), 0), (2, 5, (8,), 4), (5, 7, (8,), 8), (7, 8, (0,), 12)],
        jobs8={2: ([(0, 2, 0, 4, 14), (2, 2, 8, 2, 8)], (12, 6, 22)), 3: ([(0, 1, 0, 2, 6), (1, 1, 4, 2, 8), (2, 2, 8, 2, 8)], (12, 6, 22))},
    ),
    'descent/c4': dict(
        plan=[(0, 15, (2250,), 0), (15, 30, (2250,), 0), (30, 45, (2250,), 0), (45, 60, (2250,), 0)],
        jobs={2: ([(0, 2, 0, 410, 660), (2, 2, 1200, 410, 660)], (2400, 820, 1320)), 3: ([(0, 1, 0, 205, 330), (1, 1, 600, 205, 330), (2, 2, 1200, 410, 660)], (2400, 820, 1320))},
    ),
    'reps_first/c2': dict(
        plan=[(0, 1, (100,), 0), (1, 4, (90,), 0)],
        jobs={2: ([(0, 1, 0, 2, 4), (1, 1, 5, 6, 13)], (20, 8, 17)), 3: ([(0, 1, 0, 2, 4), (1, 1, 5, 6, 13)], (20, 8, 17))},
    ),
    'reps_last/c2': dict(
        plan=[(0, 3, (120,), 0), (3, 4, (100,), 0)],
        jobs={2: ([(0, 1, 0, 6, 13), (1, 1, 15, 2, 4)], (20, 8, 17)), 3: ([(0, 1, 0, 6, 13), (1, 1, 15, 2, 4)], (20, 8, 17))},
    ),
    'reps_every/c4': dict(
        plan=[(0, 1, (100,), 0), (1, 2, (100,), 0), (2, 3, (100,), 0), (3, 4, (100,), 0)],
        jobs={2: ([(0, 2, 0, 4, 9), (2, 2, 10, 4, 9)], (20, 8, 18)), 3: ([(0, 1, 0, 2, 4), (1, 1, 5, 2, 4), (2, 2, 10, 4, 9)], (20, 8, 17))},
    ),
    'reps_mixed/c4': dict(
        plan=[(0, 1, (100,), 0), (1, 2, (100,), 0), (2, 3, (100,), 0), (3, 4, (100,), 0)],
        jobs={2: ([(0, 2, 0, 4, 9), (2, 2, 10, 4, 9)], (20, 8, 18)), 3: ([(0, 1, 0, 2, 4), (1, 1, 5, 2, 4), (2, 2, 10, 4, 9)], (20, 8, 17))},
    ),
    'exc_every/c6': dict(
        plan=[(0, 1, (260,), 0), (1, 2, (260,), 0), (2, 3, (260,), 0), (3, 4, (260,), 0), (4, 5, (260,), 0), (5, 6, (260,), 0)],
        jobs={2: ([(0, 3, 0, 5, 12), (3, 3, 12, 5, 12)], (24, 10, 24)), 3: ([(0, 2, 0, 3, 8), (2, 2, 8, 3, 8), (4, 2, 16, 3, 8)], (24, 9, 24))},
        plan8=[(0, 1, (260,), 0), (1, 2, (260,), 4), (2, 3, (260,), 8), (3, 4, (260,), 12), (4, 5, (260,), 16), (5, 6, (260,), 20)],
        jobs8={2: ([(0, 3, 0, 5, 12), (3, 3, 12, 5, 12)], (24, 10, 24)), 3: ([(0, 2, 0, 3, 8), (2, 2, 8, 3, 8), (4, 2, 16, 3, 8)], (24, 9, 24))},
    ),
    'exc_last/c3': dict(
        plan=[(0, 5, (150,), 0), (5, 6, (260,), 0)],
        jobs={2: ([(0, 1, 0, 8, 20), (1, 1, 20, 1, 4)], (24, 9, 24)), 3: ([(0, 1, 0, 8, 20), (1, 1, 20, 1, 4)], (24, 9, 24))},
    ),
    'blocks/c16': dict(
        plan=[(0, 1, (3,), 0), (1, 2, (3,), 0), (2, 3, (3,), 0), (3, 4, (3,), 0), (4, 5, (3,), 0), (5, 6, (3,), 0), (6, 7, (3,), 0), (7, 8, (3,), 0), (8, 9, (3,), 0), (9, 10, (3,), 0), (10, 11, (3,), 0), (11, 12, (3,), 0), (12, 13, (3,), 0), (13, 14, (3,), 0), (14, 15, (3,), 0), (15, 16, (3,), 0)],
        jobs={2: ([(0, 8, 0, 685, 1040), (8, 8, 2048, 685, 1040)], (4096, 1370, 2080)), 3: ([(0, 5, 0, 428, 650), (5, 5, 1280, 428, 650), (10, 6, 2560, 514, 780)], (4096, 1370, 2080))},
        plan8=[(0, 1, (3,), 0), (1, 2, (3,), 256), (2, 3, (3,), 512), (3, 4, (3,), 768), (4, 5, (3,), 1024), (5, 6, (3,), 1280), (6, 7, (3,), 1536), (7, 8, (3,), 1792), (8, 9, (3,), 2048), (9, 10, (3,), 2304), (10, 11, (3,), 2560), (11, 12, (3,), 2816), (12, 13, (3,), 3072), (13, 14, (3,), 3328), (14, 15, (3,), 3584), (15, 16, (3,), 3840)],
        jobs8={2: ([(0, 8, 0, 685, 1040), (8, 8, 2048, 685, 1040)], (4096, 1370, 2080)), 3: ([(0, 5, 0, 428, 650), (5, 5, 1280, 428, 650), (10, 6, 2560, 514, 780)], (4096, 1370, 2080))},
    ),
    'blocks_askew/c8': dict(
        plan=[(0, 1, (3,), 0), (1, 2, (3,), 0), (2, 3, (3,), 0), (3, 4, (3,), 0), (4, 5, (3,), 0), (5, 6, (3,), 0), (6, 7, (3,), 0), (7, 8, (3,), 0)],
        jobs={2: ([(0, 4, 0, 344, 522), (4, 4, 1028, 344, 522)], (2056, 688, 1044)), 3: ([(0, 2, 0, 172, 261), (2, 3, 514, 258, 391), (5, 3, 1285, 258, 391)], (2056, 688, 1043))},
        plan8=[(0, 4, (12,), 0), (4, 8, (12,), 1028)],
        jobs8={2: ([(0, 1, 0, 344, 522), (1, 1, 1028, 344, 522)], (2056, 688, 1044)), 3: ([(0, 1, 0, 344, 522), (1, 1, 1028, 344, 522)], (2056, 688, 1044))},
    ),
})

CASES = _build()
ROUTED = _routed()

CLASSES = (["last chunk without records", "chunk without records or windows", "chunk of one read with one record", "two reads, two records, two chunks",
            "n_chunks = n_reads", "n_chunks above n_reads", "n_chunks far above n_reads", "n_chunks = 1: one piece", "all records on the last read: one piece",
            "more contexts than chunks", "jobs of unequal chunk counts", "5 chunks on one context", "8 chunks on one context", "9 chunks on one context"]
           + [f"runs: {k}" for k in (1, 2, 3, 4)]
           + ["five plain runs: routed", "five plain runs, delta4: one piece", "five grouped runs: one piece", "run absent from the first chunk",
              "run absent from a middle chunk", "run absent from the last chunk", "grouped run without records", "run inside one read",
              "reads without records at a chunk's first position", "reads without records at a chunk's last position",
              "reads without records on both sides of a boundary", "reads without windows at a chunk's ends", "a descent between two samples"]
           + ["repeats only in the first job", "repeats only in the last job", "no repeats", "repeats in every job", "fragments in every job", "close_gaps moves real data", "close_gaps moves nothing", "close_gaps moves over a gap of its full room",
              "a job's repeats equal its room", "closing offsets behind an empty chunk", "the last job is one read", "exceptions in every job",
              "exceptions only in the last chunk", "no exceptions"]
           + [f"delta4: {c}" for c in ("several chunks inside one anchor block", "a chunk inside a block another context's chunk began",
                                       "a chunk begins exactly on a block", "a chunk begins inside a block", "a chunk ends exactly on a block",
                                       "boundary moved by one read", "boundary moved by two reads", "boundary moved by three reads",
                                       "boundary dropped, the move ran to n_reads", "boundary dropped, an earlier one passed it", "odd window count")]
           + [f"routed: {c}" for c in ("n_chunks above n_reads", "every interval on one read", "reads without intervals at a chunk's ends",
                                       "records with tid == qid", "a chunk of one read", "more contexts than chunks")])

# Classes of the issue that no input reaches, with the reason read from the planner (pipeline_plan.hpp plan_chunks / place_jobs):
UNREACHABLE = {
    "first or inner chunk without records": "boundary k is the FIRST read with n_rec k / want records before it, so the read before a kept boundary has "
                                            "records, and delta4 moves boundaries forward only: every chunk but the last ends behind a read with records",
    "delta4: a chunk of zero windows between two others": "the same read has records, hence windows, and lies in the chunk its boundary closes",
    "a job of one chunk between jobs of several": "job d takes chunks [n d / 3, n (d + 1) / 3): the middle job of three never has fewer than the first",
    "a job's fragments equal its room": "with P_SHORT a read of length L is cut into at most (L - 20) / 280 + 1 fragments, its bound is L / 100 + 2",
    "fragments only in the first job, only in the last, in none": "every read has a fragment, one of length 0 included (the oracle's frag_offset)",
}


def case_id(case):
    return case.name


def by_name(name):
    return next(c for c in CASES + ROUTED if c.name == name)


class CaseModel:
    """What the model makes of a case, and what the oracle finds in every chunk and job of it."""

    def __init__(self, case):
        self.case = case
        self.plan = model_plan(case.read_len, case.run_ids, case.n_chunks, False)
        self.jobs = {n: model_jobs(self.plan, n, case.read_len) for n in CONTEXTS}
        self.events, self.plan8, self.jobs8 = [], None, {}
        if 8 in case.widths:
            self.plan8 = model_plan(case.read_len, case.run_ids, case.n_chunks, True, events=self.events)
            self.jobs8 = {n: model_jobs(self.plan8, n, case.read_len) for n in CONTEXTS}
        self.W = window_prefix(case.read_len)
        self.has_rec = [False] * case.n_reads
        for ids in case.run_ids:
            for q in ids:
                self.has_rec[q] = True

    def job_reads(self, n_ctx, plan=None):
        plan = plan or self.plan
        return [(plan[f][0], plan[f + n - 1][1]) for f, n, *_ in model_jobs(plan, n_ctx, self.case.read_len)[0]]

    def per_job(self, key, n_ctx):
        """Entries of a CSR table (rep_offset / frag_offset) or exceptions per job."""
        want = self.case.oracle()
        if key == "exc":
            deep = np.flatnonzero(want["cov"] >= 255)
            return [int(np.count_nonzero((deep >= self.W[a]) & (deep < self.W[b]))) for a, b in self.job_reads(n_ctx)]
        return [int(want[key][b] - want[key][a]) for a, b in self.job_reads(n_ctx)]

    def chunked(self, width=1):
        return self.case.plan_for(width) is not None


def holds(cls: str, case, m: CaseModel = None) -> bool:
    """Does the case fill the class, by the model and the oracle?"""
    if isinstance(case, RoutedCase):
        return _holds_routed(cls, case)
    if cls.startswith("routed: "):
        return False
    m = m or CaseModel(case)
    plan, nr, want = m.plan, case.n_reads, case.oracle
    chunked, multi = case.route == "chunked" and len(plan) >= 2, [n for n in (2, 3) if len(plan) >= 2]
    recs = lambda ch: sum(ch[2])
    absent = lambda where: chunked and any(sum(c[2][g] for c in plan) > 0 and any(plan[k][2][g] == 0 for k in where) for g in range(case.n_runs))
    reps = lambda n: m.per_job("rep_offset", n)
    frags = lambda n: m.per_job("frag_offset", n)
    rooms = lambda n: [j[3] for j in m.jobs[n][0]]

    def gaps(n):        # per job after the first: (where it wrote, where it belongs, how many)
        out, at = [], reps(n)[0]
        for j, k in zip(m.jobs[n][0][1:], reps(n)[1:]):
            rep0 = sum(rooms(n)[:m.jobs[n][0].index(j)])
            out.append((rep0, at, k))
            at += k
        return out

    if cls.startswith("delta4: "):
        if 8 not in case.widths or m.plan8 is None or len(m.plan8) < 2 or case.route != "chunked":
            return False
        p8, what = m.plan8, cls[8:]
        lo, hi = [c[3] for c in p8], [c[3] + m.W[c[1]] - m.W[c[0]] for c in p8]
        first_of = {n: {f for f, *_ in m.jobs8[n][0]} for n in CONTEXTS}
        moved = lambda d: any(why == "moved" and to - b == d for b, to, why in m.events)
        return {
            "several chunks inside one anchor block": lambda: any(lo[k] // D4_BLOCK == (hi[k + 1] - 1) // D4_BLOCK and hi[k + 1] > lo[k + 1] for k in range(len(p8) - 1)),
            "a chunk inside a block another context's chunk began": lambda: any(
                k in first_of[n] and k > 0 and lo[k] % D4_BLOCK and lo[k] // D4_BLOCK == (hi[k] - 1) // D4_BLOCK for n in (2, 3) for k in range(len(p8))),
            "a chunk begins exactly on a block": lambda: any(k > 0 and lo[k] % D4_BLOCK == 0 and hi[k] > lo[k] for k in range(len(p8))),
            "a chunk begins inside a block": lambda: any(lo[k] % D4_BLOCK and hi[k] > (lo[k] // D4_BLOCK + 1) * D4_BLOCK for k in range(len(p8))),
            "a chunk ends exactly on a block": lambda: any(k + 1 < len(p8) and hi[k] % D4_BLOCK == 0 and hi[k] > lo[k] for k in range(len(p8))),
            "boundary moved by one read": lambda: moved(1),
            "boundary moved by two reads": lambda: moved(2),
            "boundary moved by three reads": lambda: moved(3),
            "boundary dropped, the move ran to n_reads": lambda: any(why == "ran out" for _, _, why in m.events),
            "boundary dropped, an earlier one passed it": lambda: any(why == "passed" for _, _, why in m.events),
            "odd window count": lambda: m.W[-1] % 2 == 1,
        }[what]()
    if cls.startswith("runs: "):
        return chunked and case.n_runs == int(cls[6:]) and (case.forms[0] != "derived" or case.descents == case.n_runs)
    on_one = lambda k: chunked and any(len(m.jobs[n][0]) == 1 or max(j[1] for j in m.jobs[n][0]) >= k for n in (1,)) and len(plan) == k
    return {
        "last chunk without records": lambda: chunked and recs(plan[-1]) == 0 and m.W[plan[-1][1]] > m.W[plan[-1][0]],
        "chunk without records or windows": lambda: chunked and any(recs(c) == 0 and m.W[c[1]] == m.W[c[0]] for c in plan),
        "chunk of one read with one record": lambda: chunked and any(c[1] - c[0] == 1 and recs(c) == 1 for c in plan),
        "two reads, two records, two chunks": lambda: chunked and nr == 2 and case.n_rec == 2 and len(plan) == 2,
        "n_chunks = n_reads": lambda: chunked and case.n_chunks == nr,
        "n_chunks above n_reads": lambda: chunked and nr < case.n_chunks <= 2 * nr,
        "n_chunks far above n_reads": lambda: chunked and case.n_chunks >= 10 * nr,
        "n_chunks = 1: one piece": lambda: case.n_chunks == 1 and case.route == "one piece" and len(plan) == 1,
        "all records on the last read: one piece": lambda: case.n_chunks > 1 and case.route == "one piece" and len(plan) == 1 and m.has_rec == [False] * (nr - 1) + [True],
        "more contexts than chunks": lambda: chunked and len(plan) < max(CONTEXTS),
        "jobs of unequal chunk counts": lambda: chunked and any(len({j[1] for j in m.jobs[n][0]}) > 1 for n in multi),
        "5 chunks on one context": lambda: on_one(5),
        "8 chunks on one context": lambda: on_one(8),
        "9 chunks on one context": lambda: on_one(9),
        "five plain runs: routed": lambda: case.route == "routed" and "columns" in case.forms and case.descents == 5 and sampled_runs(list(case.cols[0])) is None,
        "five plain runs, delta4: one piece": lambda: case.route == "routed" and "columns" in case.forms and case.descents == 5 and 8 in case.widths,
        "five grouped runs: one piece": lambda: case.route == "one piece" and case.forms == ("grouped", "windows") and case.n_runs == 5,
        "run absent from the first chunk": lambda: absent([0]),
        "run absent from a middle chunk": lambda: len(plan) > 2 and absent(range(1, len(plan) - 1)),
        "run absent from the last chunk": lambda: absent([len(plan) - 1]),
        "grouped run without records": lambda: chunked and any(len(r) == 0 for r in case.runs) and "columns" not in case.forms,
        "run inside one read": lambda: chunked and any(len(ids) > 1 and len(set(ids)) == 1 for ids in case.run_ids) and case.n_runs > 1,
        "reads without records at a chunk's first position": lambda: chunked and any(not m.has_rec[c[0]] and recs(c) > 0 for c in plan[1:]),
        "reads without records at a chunk's last position": lambda: chunked and any(not m.has_rec[c[1] - 1] and recs(c) > 0 for c in plan),
        "reads without records on both sides of a boundary": lambda: m.plan8 is not None and any(not m.has_rec[c[0]] and not m.has_rec[c[0] - 1] for c in m.plan8[1:]),
        "reads without windows at a chunk's ends": lambda: chunked and plan[0][0] == 0 and case.read_len[0] == 0 and case.read_len[-1] == 0
                                                           and any(case.read_len[c[0]] == 0 and recs(c) > 0 for c in plan[1:]),
        "a descent between two samples": lambda: case.route == "redo" and case.n_rec > SAMPLES and case.descents == 2 and sampled_runs(list(case.cols[0])) == [0, case.n_rec]
                                                 and len(plan) >= 2,
        "repeats only in the first job": lambda: chunked and any(reps(n)[0] > 0 and not any(reps(n)[1:]) for n in multi),
        "repeats only in the last job": lambda: chunked and any(reps(n)[-1] > 0 and not any(reps(n)[:-1]) for n in multi),
        "no repeats": lambda: chunked and len(want()["rep_s"]) == 0,
        "repeats in every job": lambda: chunked and all(all(reps(n)) for n in multi),
        "fragments in every job": lambda: chunked and all(all(frags(n)) for n in multi),
        "close_gaps moves real data": lambda: chunked and any(k > 0 and at != rep0 for n in multi for rep0, at, k in gaps(n)),
        "close_gaps moves nothing": lambda: chunked and any(all(k == 0 or at == rep0 for rep0, at, k in gaps(n)) for n in multi),
        "close_gaps moves over a gap of its full room": lambda: chunked and any(reps(n)[0] == 0 and rooms(n)[0] > 0 and reps(n)[1] > 0 for n in multi),
        "a job's repeats equal its room": lambda: chunked and any(k == room > 0 for n in multi for k, room in zip(reps(n), rooms(n))),
        "closing offsets behind an empty chunk": lambda: chunked and recs(plan[-1]) == 0,
        "the last job is one read": lambda: chunked and any(b - a == 1 for n in multi for a, b in m.job_reads(n)[-1:]),
        "exceptions in every job": lambda: chunked and all(all(m.per_job("exc", n)) for n in multi),
        "exceptions only in the last chunk": lambda: chunked and bool(np.any(want()["cov"] >= 255)) and int(np.flatnonzero(want()["cov"] >= 255)[0]) >= m.W[plan[-1][0]],
        "no exceptions": lambda: chunked and not np.any(want()["cov"] >= 255),
    }[cls]()


def _holds_routed(cls, case):
    if not cls.startswith("routed: "):
        return False
    symmetric = case.oracle()["symmetric"] if case.mode < 0 else case.mode
    cnt = routed_sides(case.n_reads, case.recs, symmetric)
    bounds = {n: model_routed(case.n_reads, case.recs, symmetric, case.n_chunks, n) for n in CONTEXTS}
    chunks = lambda n: list(zip(bounds[n], bounds[n][1:]))
    return {
        "n_chunks above n_reads": lambda: case.n_chunks > case.n_reads,
        "every interval on one read": lambda: sum(1 for c in cnt if c) == 1,
        "reads without intervals at a chunk's ends": lambda: any(cnt[a] == 0 and sum(cnt[a:b]) > 0 for a, b in chunks(1)) and any(cnt[b - 1] == 0 for a, b in chunks(1)),
        "records with tid == qid": lambda: any(r[0] == r[3] for r in case.recs),
        "a chunk of one read": lambda: any(b - a == 1 and cnt[a] > 0 for a, b in chunks(1)),
        "more contexts than chunks": lambda: len(chunks(3)) < 3,
    }[cls[8:]]()
