"""CPU: the yardstick of raft_hip_repeat_overlaps_* (include/raft_hip_ovl.h) -- ``want_classes``, the header's definitions restated in
numpy -- pinned on hand-written cases with literal expected bytes, and the case lists tests/test_gpu_repeat_overlaps.py imports.

The model is deliberately not the kernel's sweep: per read the runs are sorted and merged into the disjoint pieces of their set union
(whatever order they come in), and a side's ``rep`` is the sum of its intersections with the pieces, in 64-bit integers.

Which fixture supplies which class bit (``test_the_fixtures_show_every_bit``; annotation = the goldens' exp_rep_*, which come from the
reference binary; min_anchor as in GOLDEN_ANCHORS):
    Q_REPEAT, T_REPEAT, Q_TOUCH, T_TOUCH   set and absent on each of s150_reso1, s200_smallparams, s60_ultralong, s300_default,
                                           s300_sym_shuffled and s300_nonsym_shuffled (records of every kind: 0, touch only, repeat on
                                           one side, on both)
    Q_CONTAINED, T_CONTAINED               set and absent on each of the six as well (423 .. 3280 records a side); reads that are contained
                                           only inside repeats (read_flags == 1) on all but s60_ultralong, anchored ones (3) and
                                           uncontained ones (0) on all.  The hand-written cases (HAND["contained_*"]) and ``stream``, which
                                           plants whole-read sides, supply them again
    reads with two to seven runs           s150_reso1 (85), s200_smallparams (69), s60_ultralong (21), s300_sym_shuffled (3)
"""
import json
import os

import numpy as np
import pytest
from raft_testlib import GOLDEN

Q_REPEAT, T_REPEAT, Q_TOUCH, T_TOUCH, Q_CONTAINED, T_CONTAINED = 1, 2, 4, 8, 16, 32
READ_CONTAINED, READ_ANCHORED = 1, 2
SUMMARY = ("n_records", "q_touch", "t_touch", "q_repeat", "t_repeat", "both_repeat", "q_contained", "t_contained", "reads_contained",
           "reads_repeat_contained")
I32_MAX = 2**31 - 1
# the record kernel: 256 lanes of 4 consecutive records per workgroup, at most 2048 workgroups, grid-stride beyond
LANE_RECORDS, WAVE_RECORDS, WG_RECORDS, GRID_RECORDS = 4, 256, 1024, 2048 * 1024
COUNTS = (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025, GRID_RECORDS + 5)


def union_pieces(runs):
    """The disjoint pieces of the set union of half-open intervals, ascending: sort, then merge what overlaps or touches."""
    out = []
    for s, e in sorted((int(s), int(e)) for s, e in runs if e > s):
        if out and s <= out[-1][1]:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([s, e])
    return out


def _side_rep(n_reads, rid, a, b, rep_offset, rep_s, rep_e):
    """|[a, b) intersected with U(read)| for every side, int64."""
    pieces = [union_pieces(zip(rep_s[rep_offset[r]:rep_offset[r + 1]], rep_e[rep_offset[r]:rep_offset[r + 1]])) for r in range(n_reads)]
    width = max([len(p) for p in pieces], default=0)
    S, E = np.zeros((max(n_reads, 1), max(width, 1)), np.int64), np.zeros((max(n_reads, 1), max(width, 1)), np.int64)      # (padding: the empty piece [0, 0))
    for r, p in enumerate(pieces):
        for j, (s, e) in enumerate(p):
            S[r, j], E[r, j] = s, e
    a, b = a.astype(np.int64), b.astype(np.int64)
    rep = np.zeros(a.shape, np.int64)
    count = np.array([len(p) for p in pieces] or [0], np.int64)[rid] if len(rid) else np.zeros(0, np.int64)
    for j in range(width):
        m = np.flatnonzero(count > j)                    # (the sides whose read has a piece j)
        rep[m] += np.clip(np.minimum(b[m], E[rid[m], j]) - np.maximum(a[m], S[rid[m], j]), 0, None)
    return rep


def want_classes(read_len, qid, qs, qe, tid, ts, te, symmetric, min_anchor, rep_offset, rep_s, rep_e):
    """What Engine.repeat_overlaps returns, from the definitions of include/raft_hip_ovl.h.  ts / te may be None (symmetric only)."""
    read_len, qid, qs, qe, tid = (np.asarray(x) for x in (read_len, qid, qs, qe, tid))
    rep_offset, rep_s, rep_e = np.asarray(rep_offset, np.int64), np.asarray(rep_s, np.int64), np.asarray(rep_e, np.int64)
    n_reads, n_rec = len(read_len), len(qid)
    assert ts is not None or symmetric
    L = read_len.astype(np.int64)

    def side(rid, a, b):
        span = np.maximum(b.astype(np.int64) - a.astype(np.int64), 0)
        rep = _side_rep(n_reads, rid, a, b, rep_offset, rep_s, rep_e)
        assert (rep <= span).all()
        touch = rep > 0
        return touch, touch & (span - rep < min_anchor)

    cls = np.zeros(n_rec, np.uint8)
    q_touch, q_rep = side(qid, qs, qe)
    cls |= np.where(q_touch, Q_TOUCH, 0).astype(np.uint8) | np.where(q_rep, Q_REPEAT, 0).astype(np.uint8)
    q_cont = (qs == 0) & (qe == L[qid]) & (L[tid] > L[qid])
    cls |= np.where(q_cont, Q_CONTAINED, 0).astype(np.uint8)
    if ts is not None:
        ts, te = np.asarray(ts), np.asarray(te)
        t_touch, t_rep = side(tid, ts, te)
        t_cont = (ts == 0) & (te == L[tid]) & (L[qid] > L[tid])
        cls |= (np.where(t_touch, T_TOUCH, 0) | np.where(t_rep, T_REPEAT, 0) | np.where(t_cont, T_CONTAINED, 0)).astype(np.uint8)
    else:
        t_touch = t_rep = t_cont = np.zeros(n_rec, bool)
    # the reads: query sides always, target sides of records on another read unless symmetric
    t_counts = np.zeros(n_rec, bool) if symmetric else tid != qid
    touch = np.bincount(qid[q_touch], minlength=n_reads) + np.bincount(tid[t_touch & t_counts], minlength=n_reads)
    repeat = np.bincount(qid[q_rep], minlength=n_reads) + np.bincount(tid[t_rep & t_counts], minlength=n_reads)
    flags = np.zeros(n_reads, np.uint8)
    flags[qid[q_cont]] |= READ_CONTAINED
    flags[qid[q_cont & ~t_rep]] |= READ_ANCHORED                   # the container is the target side
    flags[tid[t_cont & t_counts]] |= READ_CONTAINED
    flags[tid[t_cont & t_counts & ~q_rep]] |= READ_ANCHORED
    out = {"cls": cls, "read_touch": touch.astype(np.int32), "read_repeat": repeat.astype(np.int32), "read_flags": flags}
    out.update(n_records=n_rec, q_touch=int(q_touch.sum()), t_touch=int(t_touch.sum()), q_repeat=int(q_rep.sum()), t_repeat=int(t_rep.sum()),
               both_repeat=int((q_rep & t_rep).sum()), q_contained=int(q_cont.sum()), t_contained=int(t_cont.sum()),
               reads_contained=int((flags & READ_CONTAINED != 0).sum()), reads_repeat_contained=int((flags == READ_CONTAINED).sum()))
    return out


def same_classes(got, want, what):
    for k in ("cls", "read_touch", "read_repeat", "read_flags"):
        g = got[k].cpu().numpy() if hasattr(got[k], "is_cuda") else got[k]
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (what, k, g.dtype, g.shape)
        if not np.array_equal(g, want[k]):
            i = int(np.flatnonzero(g != want[k])[0])
            raise AssertionError(f"{what}: {k}[{i}] is {g[i]}, wanted {want[k][i]} ({int((g != want[k]).sum())} differ)")
    for k in SUMMARY:
        assert got[k] == want[k], (what, k, got[k], want[k])


def i32(*v):
    return np.array(v, np.int32).reshape(-1)


def csr(runs_per_read):
    """[[(s, e), ...] per read] -> rep_offset, rep_s, rep_e, in the order given."""
    off = np.zeros(len(runs_per_read) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in runs_per_read])
    flat = [x for r in runs_per_read for x in r]
    return off, i32(*[s for s, _ in flat]), i32(*[e for _, e in flat])


# ---- hand-written cases: name -> (read_len, [(qid, qs, qe, tid, ts, te), ...], symmetric, min_anchor, runs per read, expected class bytes,
#      expected read_touch, read_repeat, read_flags) ------------------------------------------------------------------------------------

_RUNS = [[(1000, 2000), (3000, 4000)],          # read 0: two runs
         [],                                    # read 1: none
         [(0, 500), (0, 300)],                  # read 2: tied at start 0, the longer first
         [(0, 300), (0, 500)],                  # read 3: ... the shorter first
         [(0, 8000)],                           # read 4: one run end to end
         [(100, 1100), (900, 2100), (2100, 2500)]]      # read 5: joined by their flanks, and one that touches
_LENS = [10000, 9000, 7000, 7000, 8000, 6000]
_T = (1, 0, 10)                                 # a target side on a read without runs
HAND = {
    # a side equal to a run, inside one, bridging two, touching a run by one base at either end, ending at a run's start
    "side_positions": (_LENS, [(0, 1000, 2000) + _T, (0, 1200, 1300) + _T, (0, 1500, 3500) + _T, (0, 1999, 2600) + _T, (0, 500, 1001) + _T,
                               (0, 500, 1000) + _T, (0, 2000, 3000) + _T, (0, 0, 10000) + _T],
                       False, 600, _RUNS, [5, 5, 4, 4, 5, 0, 0, 4], [6, 0, 0, 0, 0, 0], [3, 0, 0, 0, 0, 0], [0] * 6),
    # unique == min_anchor - 1 and == min_anchor: [1000, 2000) + 599 / 600 bases outside
    "anchor_boundary": (_LENS, [(0, 401, 2000) + _T, (0, 400, 2000) + _T, (1, 0, 10, 0, 1000, 2599), (1, 0, 10, 0, 1000, 2600)],
                        False, 600, _RUNS, [5, 4, 10, 8], [4, 0, 0, 0, 0, 0], [2, 0, 0, 0, 0, 0], [0] * 6),
    "min_anchor_1": (_LENS, [(0, 1000, 2000) + _T, (0, 1000, 2001) + _T, (0, 999, 2000) + _T], False, 1, _RUNS, [5, 4, 4], [3, 0, 0, 0, 0, 0],
                     [1, 0, 0, 0, 0, 0], [0] * 6),
    "min_anchor_max": (_LENS, [(0, 1999, I32_MAX) + _T, (0, -I32_MAX, 1001) + _T, (1, 0, 9000, 0, 0, 10000)], False, I32_MAX, _RUNS,
                       [5, 4, 2 | 8 | 16], [3, 0, 0, 0, 0, 0], [2, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0]),
    # qe <= qs: span 0; a span of 2^31 - 1 and beyond it (negative start)
    "empty_and_huge_spans": (_LENS, [(0, 1500, 1500) + _T, (0, 1800, 1200) + _T, (0, 0, I32_MAX) + _T, (0, -5, I32_MAX) + _T, (4, 0, I32_MAX) + _T],
                             False, 1000, _RUNS, [0, 0, 4, 4, 4], [2, 0, 0, 0, 1, 0], [0] * 6, [0] * 6),
    # runs tied at start 0 in both orders give the same union; a read that is one run; runs joined by flanks are one piece
    "unions": (_LENS, [(2, 0, 500) + _T, (3, 0, 500) + _T, (2, 250, 700) + _T, (3, 250, 700) + _T, (4, 0, 8000, 5, 100, 2500),
                       (5, 0, 2600, 4, 7999, 8001), (5, 2500, 2600, 5, 2499, 2500)],
               False, 201, _RUNS, [5, 5, 5, 5, 15, 5 | 10, 10], [0, 0, 2, 2, 2, 2], [0, 0, 2, 2, 2, 2], [0] * 6),
    # containment: equal lengths never flag; tid == qid never flags and its target side counts for no read
    "contained_equal_and_self": ([7000, 7000, 8000], [(0, 0, 7000, 1, 0, 7000), (2, 0, 8000, 2, 0, 8000)], False, 1000,
                                 [[], [], [(0, 8000)]], [0, 15], [0, 0, 1], [0, 0, 1], [0, 0, 0]),
    # a read contained twice, once anchored and once not, in both orders; the same through target sides
    "contained_twice_query": ([5000, 9000, 9000, 5000], [(0, 0, 5000, 1, 1000, 6000), (0, 0, 5000, 2, 1000, 6000),
                                                         (3, 0, 5000, 2, 1000, 6000), (3, 0, 5000, 1, 1000, 6000)],
                              False, 1000, [[], [(500, 7000)], [], []], [16 | 10, 16, 16, 16 | 10], [0, 2, 0, 0], [0, 2, 0, 0], [3, 0, 0, 3]),
    "contained_only_in_repeats": ([5000, 9000, 9000, 5000], [(0, 0, 5000, 1, 1000, 6000), (3, 0, 5000, 2, 1000, 6000)], False, 1000,
                                  [[], [(500, 7000)], [], []], [16 | 10, 16], [0, 1, 0, 0], [0, 1, 0, 0], [1, 0, 0, 3]),
    "contained_twice_target": ([5000, 9000, 9000, 5000], [(1, 1000, 6000, 0, 0, 5000), (2, 1000, 6000, 0, 0, 5000),
                                                          (2, 1000, 6000, 3, 0, 5000), (1, 1000, 6000, 3, 0, 5000)],
                               False, 1000, [[], [(500, 7000)], [], []], [32 | 5, 32, 32, 32 | 5], [0, 2, 0, 0], [0, 2, 0, 0], [3, 0, 0, 3]),
    # symmetric: target sides are classified in the byte but count for no read, and T_CONTAINED flags nobody
    "symmetric_counts_query_sides": ([5000, 9000], [(1, 1000, 6000, 0, 0, 5000), (0, 0, 5000, 1, 1000, 6000)], True, 1000,
                                     [[(0, 5000)], [(500, 7000)]], [32 | 15, 16 | 15], [1, 1], [1, 1], [1, 0]),
}


def hand_case(name):
    """-> (columns as Engine.repeat_overlaps takes them, symmetric, min_anchor, (rep_offset, rep_s, rep_e), expected dict of arrays)"""
    lens, recs, sym, anchor, runs, cls, touch, repeat, flags = HAND[name]
    cols = [i32(*lens)] + [i32(*[r[k] for r in recs]) for k in range(6)]
    exp = {"cls": np.array(cls, np.uint8), "read_touch": i32(*touch), "read_repeat": i32(*repeat), "read_flags": np.array(flags, np.uint8)}
    return cols, sym, anchor, csr(runs), exp


@pytest.mark.parametrize("name", sorted(HAND))
def test_the_model_on_hand_written_cases(name):
    cols, sym, anchor, rep, exp = hand_case(name)
    got = want_classes(*cols, sym, anchor, *rep)
    for k, v in exp.items():
        assert np.array_equal(got[k], v), (name, k, list(got[k]), list(v))
    assert got["n_records"] == len(cols[1]) and got["q_repeat"] == int((exp["cls"] & 1 != 0).sum()) and got["both_repeat"] == int((exp["cls"] & 3 == 3).sum())
    assert got["reads_contained"] == int((exp["read_flags"] & 1).sum()) and got["reads_repeat_contained"] == int((exp["read_flags"] == 1).sum())


def test_the_model_without_target_columns():
    cols, _, anchor, rep, exp = hand_case("symmetric_counts_query_sides")
    got = want_classes(*cols[:5], None, None, True, anchor, *rep)
    assert list(got["cls"]) == [5, 16 | 5] and list(got["read_flags"]) == [3, 0]       # (no T_REPEAT to be had: the container counts as an anchor)
    assert got["t_touch"] == got["t_repeat"] == got["t_contained"] == 0


def test_union_pieces():
    assert union_pieces([(0, 300), (0, 500)]) == union_pieces([(0, 500), (0, 300)]) == [[0, 500]]
    assert union_pieces([(100, 1100), (900, 2100), (2100, 2500), (3000, 3000), (4000, 4001)]) == [[100, 2500], [4000, 4001]]
    assert union_pieces([(100, 5000), (200, 1000), (4000, 6000)]) == [[100, 6000]]      # rep_e need not ascend


# ---- generated streams -------------------------------------------------------------------------------------------------------------------

def stream_reads(seed=11, n_reads=53):
    """Reads with 0, 1, 2 and 40 runs; runs that overlap through flanks, touch, nest (rep_e descending), tie at start 0 in both orders; a
    read that is one run end to end.  rep_s ascends within every read."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(3000, 30000, n_reads).astype(np.int32)
    runs = []
    for r in range(n_reads):
        L, kind = int(lens[r]), r % 9
        if kind in (0, 3, 6):
            runs.append([])
        elif kind == 1:
            s = int(rng.integers(0, L - 1500)); runs.append([(s, s + int(rng.integers(300, 1500)))])
        elif kind == 2:
            runs.append([(200, 900), (1500, 2600)] if r % 2 else [(200, 1600), (1400, 2600), (2600, 2800)])
        elif kind == 4:
            step = L // 41
            runs.append([(k * step + 10, k * step + 10 + step // 2) for k in range(40)])
        elif kind == 5:
            runs.append([(0, 500), (0, 300), (1000, 1400)] if r % 2 else [(0, 300), (0, 500), (1000, 1400)])
        elif kind == 7:
            runs.append([(0, L)])
        else:
            runs.append([(100, 2500), (200, 1000), (2400, 2700)])
    return lens, runs


def stream(n_rec, seed=5):
    """n_rec records over stream_reads(): the query column in sorted runs of one id (lengths 1 .. 6 and 1 .. 700: within a lane, across lanes, waves and
    workgroups), targets anywhere; sides drawn from run edges and random positions; whole-read sides, which plant containment."""
    lens, runs = stream_reads()
    n_reads = len(lens)
    rng = np.random.default_rng(seed + n_rec)
    ids = []
    while len(ids) < n_rec:
        ids += [int(rng.integers(0, n_reads))] * int(rng.integers(1, 700) if rng.random() < 0.2 else rng.integers(1, 7))
    qid = np.array(ids[:n_rec], np.int32)
    tid = rng.integers(0, n_reads, n_rec).astype(np.int32)

    def sides(rid):
        L = lens[rid].astype(np.int64)
        a = (rng.random(n_rec) * L).astype(np.int64)
        b = a + (rng.random(n_rec) * (L - a)).astype(np.int64)
        kind = rng.integers(0, 8, n_rec)
        edges_s = np.array([runs[r][0][0] if runs[r] else 0 for r in range(n_reads)], np.int64)
        edges_e = np.array([runs[r][0][1] if runs[r] else 0 for r in range(n_reads)], np.int64)
        a = np.where(kind == 0, 0, a); b = np.where(kind == 0, L, b)                               # the whole read
        a = np.where(kind == 1, edges_s[rid], a); b = np.where(kind == 1, edges_e[rid], b)         # the first run itself
        a = np.where(kind == 2, np.maximum(edges_s[rid] - 300, 0), a); b = np.where(kind == 2, edges_s[rid] + 1, b)   # touches it by one base
        b = np.where(kind == 3, np.maximum(edges_s[rid], a), b)                                    # ends where it starts: no touch
        return a.astype(np.int32), b.astype(np.int32)

    qs, qe = sides(qid)
    ts, te = sides(tid)
    cols = [lens, qid, qs, qe, tid, ts, te]
    return cols, csr(runs)


def joined_run(n_rec, flagged):
    """A sorted run of one id over n_rec records, every side inside the read's one run (flagged) or on reads without any (not): the
    tallies' joins within the lane, across the wave and across workgroups either add everything or nothing."""
    lens = i32(9000, 9000, 7000, 7000)
    rep = csr([[(0, 9000)], [(0, 9000)], [], []])
    q = 0 if flagged else 2
    rng = np.random.default_rng(n_rec)
    a = rng.integers(0, 3000, n_rec).astype(np.int32)
    b = (a + rng.integers(1, 3000, n_rec)).astype(np.int32)
    cols = [lens, np.full(n_rec, q, np.int32), a, b, np.full(n_rec, q + 1, np.int32), a.copy(), b.copy()]
    return cols, rep


JOIN_COUNTS = (LANE_RECORDS + 1, WAVE_RECORDS - 1, WAVE_RECORDS + 3, WG_RECORDS + 7, 3 * WG_RECORDS + 1)
GOLDEN_ANCHORS = {"s150_reso1": 40, "s200_smallparams": 100, "s60_ultralong": 1500, "s300_default": 2000, "s300_sym_shuffled": 2000,
                  "s300_nonsym_shuffled": 2000}


def golden_case(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cols = [z[k] for k in ("read_len", "qid", "qs", "qe", "tid", "ts", "te")]
    return cols, (z["exp_rep_offset"].astype(np.int64), z["exp_rep_s"], z["exp_rep_e"])


def golden_params(name):
    return json.load(open(os.path.join(GOLDEN, "manifest.json")))["synthetic"][name]["params"]


def test_the_fixtures_show_every_bit():
    """On every golden used, each of the six class bits is set on some record and absent on another, and reads with several runs are
    among the sides; the hand-written cases and the generated stream show every bit again."""
    multi = 0
    for name, anchor in GOLDEN_ANCHORS.items():
        cols, rep = golden_case(name)
        w = want_classes(*cols, False, anchor, *rep)
        for bit in (Q_REPEAT, T_REPEAT, Q_TOUCH, T_TOUCH, Q_CONTAINED, T_CONTAINED):
            assert 0 < int((w["cls"] & bit != 0).sum()) < len(w["cls"]), (name, bit)
        assert {0, 3} <= set(w["read_flags"].tolist()) and (name == "s60_ultralong" or 1 in w["read_flags"]), name
        assert (w["cls"] == 0).any() and (w["cls"] & 3 == 3).any(), name
        assert (w["cls"] & 5 == 4).any() and (w["cls"] & 10 == 8).any(), name                  # touching without lying inside
        multi += int((np.diff(rep[0]) >= 2).sum())
    assert multi >= 150
    seen = 0
    for name in HAND:
        seen |= int(np.bitwise_or.reduce(hand_case(name)[4]["cls"]))
    assert seen == 63
    cols, rep = stream(1023)
    w = want_classes(*cols, False, 300, *rep)
    assert int(np.bitwise_or.reduce(w["cls"])) == 63 and (w["cls"] == 0).any()
    assert {1, 3} <= set(w["read_flags"].tolist()) and 0 in w["read_flags"]


def test_the_generated_reads_are_what_the_cases_need():
    lens, runs = stream_reads()
    assert {0, 1, 2, 3, 40} <= {len(r) for r in runs}
    for r in runs:
        assert [s for s, _ in r] == sorted(s for s, _ in r)                                        # rep_s ascends; rep_e need not
    assert any(any(r[k][1] > r[k + 1][1] for k in range(len(r) - 1)) for r in runs)
    assert any(r == [(0, int(L))] for r, L in zip(runs, lens))
    assert [(0, 500), (0, 300)] in [r[:2] for r in runs] and [(0, 300), (0, 500)] in [r[:2] for r in runs]
    cols, _ = stream(5000)
    run_lengths = np.diff(np.flatnonzero(np.r_[True, np.diff(cols[1]) != 0, True]))
    assert run_lengths.max() > WAVE_RECORDS and run_lengths.min() < LANE_RECORDS
