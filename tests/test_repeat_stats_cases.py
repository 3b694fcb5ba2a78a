"""CPU: the model and the cases of the per-repeat table (include/raft_hip_rst.h; raft_amd/csrc/repeat_stats.hpp).

repeat_stats_model is a brute force over every (counted side, run) pair, with the window ranges taken from an int32 coverage array; it is
written from the header and from none of the kernels' arithmetic (no digest, no hull, no walk that stops early, no join).  The case
builders give: a lattice of sides around every run boundary, reads with 0, 1, 2, 17 and 130 runs, runs joined by their flanks, three runs
tied at start 0 with descending ends, an EMPTY run between two real ones, a run [0, len), explicit runs with s < 0 and e > len, a record
of a read with itself, under symmetric 0 and 1.  A census taken from the cases alone fails on an empty class; the unit constants the GPU
cases are built on are read back from repeat_stats.hpp; and eight one-line mistakes in the model are each shown caught on a named case."""
import os
import re

import numpy as np
import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "raft_amd", "csrc")
EMPTY, AT_START, AT_END = 1, 2, 4
COUNTS = ("run_touch", "run_span", "run_inside")
COVERAGE = ("run_windows", "run_cov_min", "run_cov_max", "run_high", "run_cov_sum")
ARRAYS = COUNTS + COVERAGE + ("run_flags",)
SUMMARY = ("n_runs", "runs_empty", "runs_interior", "runs_touched", "runs_spanned", "interior_spanned", "sides_touch", "sides_span", "sides_inside",
           "windows", "cov_sum")
# the record kernel: 256 lanes of 4 consecutive records per workgroup; the coverage kernel: a wave takes 64 * 4 windows per step
LANE_RECORDS, WAVE_RECORDS, WG_RECORDS, COV_STEP = 4, 256, 1024, 256
MISTAKES = ("span_strict", "inside_strict", "self_target_counted", "j1_floor", "no_clip_to_W", "empty_run_counted", "target_under_symmetric",
            "max_of_nothing")


def i32(*v):
    return np.array(v, np.int32).reshape(-1)


def csr(runs_per_read):
    """[[(s, e), ...] per read] -> rep_offset, rep_s, rep_e, in the order given."""
    off = np.zeros(len(runs_per_read) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in runs_per_read])
    flat = [x for r in runs_per_read for x in r]
    return off, i32(*[s for s, _ in flat]), i32(*[e for _, e in flat])


def counted_sides(qid, qs, qe, tid, ts, te, symmetric, mistake=None):
    """(read, a, b) of every side the census counts: the query side of every record and, unless symmetric, the target side of every
    record with tid != qid."""
    rid, a, b = [np.asarray(qid, np.int64)], [np.asarray(qs, np.int64)], [np.asarray(qe, np.int64)]
    if (not symmetric or mistake == "target_under_symmetric") and ts is not None:
        keep = np.ones(len(qid), bool) if mistake == "self_target_counted" else np.asarray(tid) != np.asarray(qid)
        rid.append(np.asarray(tid, np.int64)[keep]); a.append(np.asarray(ts, np.int64)[keep]); b.append(np.asarray(te, np.int64)[keep])
    return np.concatenate(rid), np.concatenate(a), np.concatenate(b)


def repeat_stats_model(read_len, qid, qs, qe, tid, ts, te, symmetric, rep_offset, rep_s, rep_e, threshold=0, cov_offset=None, cov=None, reso=None,
                       mistake=None):
    """What Engine.repeat_stats returns, from the definitions of include/raft_hip_rst.h.  qid .. te may all be None (no records); ts / te
    may be None under symmetric.  threshold >= 1 needs the pass's cov_offset, cov (int32) and reso.  `mistake`: one of MISTAKES, planted."""
    assert mistake is None or mistake in MISTAKES
    L = np.asarray(read_len, np.int64)
    off, S, E = np.asarray(rep_offset, np.int64), np.asarray(rep_s, np.int64), np.asarray(rep_e, np.int64)
    n_reads, n_rep = len(L), len(S)
    assert off[0] == 0 and off[-1] == n_rep and (np.diff(off) >= 0).all() and len(off) == n_reads + 1
    if qid is None:
        rid = a = b = np.zeros(0, np.int64)
    else:
        assert ts is not None or symmetric
        rid, a, b = counted_sides(qid, qs, qe, tid, ts, te, symmetric, mistake)
        assert ((rid >= 0) & (rid < n_reads)).all()
    real = b > a
    rid, a, b = rid[real], a[real], b[real]
    out = {k: np.zeros(n_rep, np.int32) for k in COUNTS}
    out["run_flags"] = np.zeros(n_rep, np.uint8)
    pairs = {"touch_only": 0, "span_not_inside": 0, "inside_not_span": 0, "all_three": 0}
    by_read = [np.flatnonzero(rid == r) for r in range(n_reads)] if n_rep else []
    for r in range(n_reads):
        for k in range(off[r], off[r + 1]):
            s, e = S[k], E[k]
            out["run_flags"][k] = (EMPTY if e <= s else 0) | (AT_START if s <= 0 else 0) | (AT_END if e >= L[r] else 0)
            if e <= s and mistake != "empty_run_counted":
                continue
            x, y = a[by_read[r]], b[by_read[r]]
            touch = (x < e) & (y > s)
            span = ((x < s) & (y > e)) if mistake == "span_strict" else ((x <= s) & (y >= e))
            inside = ((x > s) & (y < e)) if mistake == "inside_strict" else ((x >= s) & (y <= e))
            out["run_touch"][k], out["run_span"][k], out["run_inside"][k] = touch.sum(), span.sum(), inside.sum()
            pairs["touch_only"] += int((touch & ~span & ~inside).sum()); pairs["span_not_inside"] += int((span & ~inside).sum())
            pairs["inside_not_span"] += int((inside & ~span).sum()); pairs["all_three"] += int((span & inside).sum())
    for k in COVERAGE:
        out[k] = None
    if threshold >= 1:
        cov_offset, cov = np.asarray(cov_offset, np.int64), np.asarray(cov)
        assert cov.dtype == np.int32 and len(cov_offset) == n_reads + 1 and reso >= 1
        out.update({k: np.zeros(n_rep, np.int64 if k == "run_cov_sum" else np.int32) for k in COVERAGE})
        for r in range(n_reads):
            W = int(cov_offset[r + 1] - cov_offset[r])
            row = cov[cov_offset[r]:cov_offset[r + 1]].astype(np.int64)
            for k in range(off[r], off[r + 1]):
                s, e = int(S[k]), int(E[k])
                j0 = max(s, 0) // reso
                j1 = e // reso if mistake == "j1_floor" else -(-e // reso)
                if mistake != "no_clip_to_W":
                    j1 = min(j1, W)
                n = 0 if e <= s else max(j1 - j0, 0)
                out["run_windows"][k] = n
                if mistake == "no_clip_to_W":
                    n = min(n, max(W - j0, 0))               # (the planted mistake is in the count; the model still reads its own row only)
                w = row[j0:j0 + n]
                if n > 0:
                    out["run_cov_sum"][k], out["run_cov_min"][k], out["run_cov_max"][k] = w.sum(), w.min(), w.max()
                    out["run_high"][k] = int((w >= threshold).sum())
                elif mistake == "max_of_nothing":
                    out["run_cov_max"][k] = -2**31
    f = out["run_flags"]
    out.update(n_runs=n_rep, runs_empty=int((f & EMPTY != 0).sum()), runs_interior=int((f == 0).sum()), runs_touched=int((out["run_touch"] > 0).sum()),
               runs_spanned=int((out["run_span"] > 0).sum()), interior_spanned=int(((f == 0) & (out["run_span"] > 0)).sum()),
               sides_touch=int(out["run_touch"].astype(np.int64).sum()), sides_span=int(out["run_span"].astype(np.int64).sum()),
               sides_inside=int(out["run_inside"].astype(np.int64).sum()),
               windows=0 if threshold < 1 else int(out["run_windows"].astype(np.int64).sum()), cov_sum=0 if threshold < 1 else int(out["run_cov_sum"].sum()))
    out["pairs"] = pairs
    return out


def same_stats(got, want, what):
    for k in ARRAYS:
        if want[k] is None:
            assert got[k] is None, (what, k)
            continue
        g = got[k]
        assert isinstance(g, np.ndarray) and g.dtype == want[k].dtype and g.shape == want[k].shape, (what, k, getattr(g, "dtype", None), getattr(g, "shape", None))
        if not np.array_equal(g, want[k]):
            i = int(np.flatnonzero(g != want[k])[0])
            raise AssertionError(f"{what}: {k}[{i}] is {g[i]}, wanted {want[k][i]} ({int((g != want[k]).sum())} differ)")
    for k in SUMMARY:
        assert got[k] == want[k], (what, k, got[k], want[k])


def where_of(flags):
    return ["empty" if f & EMPTY else "whole" if f & 6 == 6 else "head" if f & AT_START else "tail" if f & AT_END else "interior" for f in flags]


# ---- the reads of the cases ---------------------------------------------------------------------------------------------------------------

R_NONE, R_ONE, R_TWO, R_17, R_130, R_FLANKS, R_TIED, R_GAP, R_WHOLE, R_OUTSIDE, R_NONE2, R_ONE_REAL, R_ONLY_EMPTY = range(13)


def case_reads():
    """-> read_len, runs per read.  rep_s ascends within every read; rep_e need not."""
    lens = [4000, 5000, 6000, 8000, 30000, 6000, 7000, 5000, 3210, 2000, 1234, 3000, 2500]
    runs = [[] for _ in lens]
    runs[R_ONE] = [(1000, 2000)]
    runs[R_TWO] = [(500, 1500), (3000, 4000)]
    runs[R_17] = [(100 + 400 * i, 350 + 400 * i) for i in range(17)]
    runs[R_130] = [(50 + 200 * i, 170 + 200 * i) for i in range(130)]
    runs[R_FLANKS] = [(100, 1100), (900, 2100), (2100, 2500)]              # joined by their flanks, and one that touches
    runs[R_TIED] = [(0, 900), (0, 600), (0, 300)]                           # tied at start 0, the ends descending
    runs[R_GAP] = [(200, 700), (900, 900), (1200, 1800)]                    # an EMPTY run between two real ones
    runs[R_WHOLE] = [(0, 3210)]
    runs[R_OUTSIDE] = [(-50, 400), (1700, 2080)]                            # (explicit arrays only: the engine clamps)
    runs[R_ONE_REAL] = [(500, 500), (800, 1600), (1700, 1650)]              # one real run between EMPTY ones
    runs[R_ONLY_EMPTY] = [(300, 300), (700, 600)]
    return i32(*lens), runs


def lattice_sides(runs):
    """Around every run: a in {s - 1, s, s + 1} x b in {e - 1, e, e + 1}, a side wholly left, one wholly right, one ending at s, one
    beginning at e, and two with b <= a."""
    out = []
    for s, e in runs:
        out += [(a, b) for a in (s - 1, s, s + 1) for b in (e - 1, e, e + 1)]
        out += [(s - 20, s - 5), (e + 5, e + 20), (s - 9, s), (e, e + 9), (s + 3, s + 3), (e, s)]
    return out


def lattice_case():
    """Every lattice side of every run once as a query side (the target side on a read without runs) and once as a target side (the query
    side on a read without runs), and a record of every read with itself whose target side equals a run.  -> columns, (rep_offset, rep_s, rep_e)"""
    lens, runs = case_reads()
    rec = []
    for r, rr in enumerate(runs):
        for a, b in lattice_sides(rr):
            rec.append((r, a, b, R_NONE, 0, 10))
            rec.append((R_NONE2, 5, 15, r, a, b))
        for s, e in rr[:2]:
            rec.append((r, s + 1, e + 1, r, s, e))                           # a read with itself: the target side is not counted
    cols = [lens] + [i32(*[x[k] for x in rec]) for k in range(6)]
    return cols, csr(runs)


def census(cols, sym, rep, want):
    """The classes the cases must show, from the cases and the model's output alone."""
    off, S, E = rep
    rid, a, b = counted_sides(*cols[1:], sym)
    n_runs = np.diff(off)
    multi = n_runs[rid] > 1
    last_s = np.array([S[off[r + 1] - 1] if n_runs[r] else 0 for r in range(len(n_runs))], np.int64)
    real = b > a
    seen = dict(want["pairs"])
    seen.update({w: where_of(want["run_flags"]).count(w) for w in ("interior", "head", "tail", "whole", "empty")})
    seen["walk_breaks_early"] = int((multi & real & (b <= last_s[rid])).sum())          # some later run has s >= b
    seen["walk_reaches_last_run"] = int((multi & real & (b > last_s[rid])).sum())
    seen["self_record"] = int((cols[1] == cols[4]).sum())
    seen["empty_side"] = int((~real).sum())
    seen["run_counts"] = int({0, 1, 2, 17, 130} <= set(n_runs.tolist()))
    return seen


def synthetic_coverage(lens, reso, seed=3):
    """An int32 coverage array over ceil(len / reso) windows per read -- what a pass would hold, here drawn at random."""
    rng = np.random.default_rng(seed)
    W = -(-np.asarray(lens, np.int64) // reso)
    off = np.concatenate([[0], np.cumsum(W)]).astype(np.int64)
    return off, rng.integers(0, 40, int(off[-1])).astype(np.int32)


# ---- generated streams for the GPU cases -----------------------------------------------------------------------------------------------------

def stream(n_rec, seed=5):
    """n_rec records over case_reads(): the query column in sorted runs of one id (lengths 1 .. 6 and 1 .. 700: within a lane, across
    lanes, waves and workgroups), targets anywhere; sides drawn from run edges (one off either way) and random positions."""
    lens, runs = case_reads()
    n_reads = len(lens)
    rng = np.random.default_rng(seed + n_rec)
    ids = []
    while len(ids) < n_rec:
        ids += [int(rng.integers(0, n_reads))] * int(rng.integers(1, 700) if rng.random() < 0.2 else rng.integers(1, 7))
    qid = np.array(ids[:n_rec], np.int32)
    tid = rng.integers(0, n_reads, n_rec).astype(np.int32)

    def sides(rid):
        a = (rng.random(rid.size) * lens[rid]).astype(np.int64)
        b = a + 1 + (rng.random(rid.size) * 2500).astype(np.int64)
        for i in np.flatnonzero(rng.random(rid.size) < 0.5):
            rr = runs[int(rid[i])]
            if rr:
                s, e = rr[int(rng.integers(0, len(rr)))]
                s2, e2 = rr[int(rng.integers(0, len(rr)))]
                a[i], b[i] = min(s, s2) + int(rng.integers(-1, 2)), max(e, e2) + int(rng.integers(-1, 2))
                if rng.random() < 0.3:
                    a[i], b[i] = s + int(rng.integers(0, 2)), e - int(rng.integers(0, 2))
        return a.astype(np.int32), b.astype(np.int32)
    qs, qe = sides(qid)
    ts, te = sides(tid)
    return [lens, qid, qs, qe, tid, ts, te], csr(runs)


STREAKS = (1, 2, 4, 255, 256, 257, 1023, 1024, 1025, 70000)


def streak_case(n, column, lead=3):
    """n consecutive records on one single-run read, in the query or the target column, set between `lead` and 3 records of other reads.
    The 70,000 (past 16 bits) are all equal to the run: touch + span + inside each; shorter streaks mix the classes."""
    lens = i32(4000, 5000, 6000, 5000)
    runs = [[], [(1000, 2000)], [(500, 1500), (3000, 4000)], [(700, 900)]]
    rng = np.random.default_rng(n)
    if n >= 70000:
        a, b = np.full(n, 1000, np.int64), np.full(n, 2000, np.int64)
    else:
        a, b = 1000 + rng.integers(-2, 3, n), 2000 + rng.integers(-2, 3, n)
    other = [(3, 700, 900), (2, 400, 4100), (3, 650, 950), (2, 3000, 4000), (3, 800, 850), (0, 5, 50)]
    hot = np.r_[[x[0] for x in other[:lead]], np.full(n, 1), [x[0] for x in other[3:]]]
    ha = np.r_[[x[1] for x in other[:lead]], a, [x[1] for x in other[3:]]]
    hb = np.r_[[x[2] for x in other[:lead]], b, [x[2] for x in other[3:]]]
    cold, ca, cb = np.zeros(hot.size), np.full(hot.size, 5), np.full(hot.size, 60)
    q, t = ((hot, ha, hb), (cold, ca, cb)) if column == "q" else ((cold, ca, cb), (hot, ha, hb))
    return [lens] + [np.asarray(x, np.int32) for x in (*q, *t)], csr(runs)


# ---- the tests ------------------------------------------------------------------------------------------------------------------------------

def test_the_constants_the_cases_are_built_on():
    rst, shared = open(os.path.join(CSRC, "repeat_stats.hpp")).read(), open(os.path.join(CSRC, "record_stream.hpp")).read()

    def one(pattern, text):
        m = re.findall(pattern, text)
        assert len(m) == 1, (pattern, m)
        return m[0]
    assert int(one(r"constexpr int kStreamLaneRecords = (\d+);", shared)) == LANE_RECORDS
    threads = int(one(r"constexpr int kStreamThreads = (\d+);", shared))
    one(r"constexpr int kStreamWaveRecords = kStreamLaneRecords \* kWave;", shared)
    one(r"const long long per_step = \(long long\)kStreamThreads \* kStreamLaneRecords;", shared)
    # the record kernel has no launch constant of its own: the shared ones, and the packed weight's field is sized by the shared wave
    one(r'#include "record_stream.hpp"', rst)
    one(r"__launch_bounds__\(kStreamThreads\) void rst_side_kernel", rst)
    assert not re.search(r"constexpr int kRst(Threads|LaneRecords|WaveRecords|BlockRecords|MaxBlocks)\b", rst)
    one(r"static_assert\(kStreamWaveRecords < \(1 << kRstFieldBits\)", rst)
    assert LANE_RECORDS * 64 == WAVE_RECORDS and LANE_RECORDS * threads == WG_RECORDS
    assert int(one(r"constexpr int kRstCovVec = (\d+);", rst)) * 64 == COV_STEP
    one(r"constexpr int kRstCovStep = kRstCovVec \* kWave;", rst)
    assert WAVE_RECORDS < 1 << int(one(r"constexpr int kRstFieldBits = (\d+);", rst))
    hdr = open(os.path.join(CSRC, "..", "..", "include", "raft_hip_rst.h")).read()
    assert [int(one(rf"#define RAFT_HIP_RST_{n}\s+(\d+)", hdr)) for n in ("EMPTY", "AT_START", "AT_END")] == [EMPTY, AT_START, AT_END]


def test_the_model_on_hand_written_numbers():
    """One read, runs [1000, 2000) and [3000, 4000), sides written out with their classes."""
    lens, rep = i32(5000, 100), csr([[(1000, 2000), (3000, 4000)], []])
    rec = [(0, 1000, 2000), (0, 999, 2001), (0, 1001, 1999), (0, 1500, 3500), (0, 0, 5000), (0, 2000, 3000), (0, 1999, 3001), (0, 500, 1000), (0, 1200, 1200)]
    cols = [lens] + [i32(*[r[k] for r in rec]) for k in range(3)] + [i32(*[1] * len(rec)), i32(*[0] * len(rec)), i32(*[10] * len(rec))]
    w = repeat_stats_model(*cols, False, *rep)
    assert list(w["run_touch"]) == [6, 3] and list(w["run_span"]) == [3, 1] and list(w["run_inside"]) == [2, 0]
    assert list(w["run_flags"]) == [0, 0] and w["runs_interior"] == 2 and w["interior_spanned"] == 2 and w["sides_touch"] == 9
    assert w["pairs"] == {"touch_only": 4, "span_not_inside": 3, "inside_not_span": 1, "all_three": 1}
    off, cov = np.array([0, 10, 11], np.int64), i32(1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 99)
    w = repeat_stats_model(*cols, False, *rep, threshold=5, cov_offset=off, cov=cov, reso=500)
    assert list(w["run_windows"]) == [2, 2] and list(w["run_cov_sum"]) == [3 + 4, 7 + 8] and list(w["run_cov_min"]) == [3, 7]
    assert list(w["run_cov_max"]) == [4, 8] and list(w["run_high"]) == [0, 2] and w["windows"] == 4 and w["cov_sum"] == 22
    w = repeat_stats_model(*cols, False, *csr([[(1001, 2001), (4400, 7000)], []]), threshold=5, cov_offset=off, cov=cov, reso=500)
    assert list(w["run_windows"]) == [3, 2] and list(w["run_cov_sum"]) == [3 + 4 + 5, 9 + 10] and list(w["run_flags"]) == [0, AT_END]


@pytest.mark.parametrize("sym", (False, True))
def test_the_cases_show_every_class(sym):
    cols, rep = lattice_case()
    want = repeat_stats_model(*cols, sym, *rep)
    seen = census(cols, sym, rep, want)
    assert all(v > 0 for v in seen.values()), seen
    lens, runs = case_reads()
    k = int(rep[0][R_GAP])
    assert want["run_flags"][k + 1] == EMPTY and want["run_touch"][k + 1] == 0 and want["run_touch"][k] > 0 and want["run_touch"][k + 2] > 0
    k = int(rep[0][R_TIED])
    assert list(rep[1][k:k + 3]) == [0, 0, 0] and list(np.diff(rep[2][k:k + 3]) < 0) == [True, True]
    assert where_of(want["run_flags"][rep[0][R_OUTSIDE]:rep[0][R_OUTSIDE] + 2]) == ["head", "tail"]
    assert where_of(want["run_flags"][rep[0][R_WHOLE]:rep[0][R_WHOLE] + 1]) == ["whole"]
    if sym:                                                              # half the lattice is target sides: they count only without the flag
        assert want["sides_touch"] < repeat_stats_model(*cols, False, *rep)["sides_touch"]
    for r in runs:
        assert [s for s, _ in r] == sorted(s for s, _ in r)
    cols, rep = stream(5000)
    streaks = np.diff(np.flatnonzero(np.r_[True, np.diff(cols[1]) != 0, True]))
    assert streaks.max() > WAVE_RECORDS and streaks.min() < LANE_RECORDS
    assert all(v > 0 for v in census(cols, sym, rep, repeat_stats_model(*cols, sym, *rep)).values())


def test_streaks_are_what_they_say():
    for n in STREAKS[:-1]:
        for column in "qt":
            cols, rep = streak_case(n, column)
            want = repeat_stats_model(*cols, False, *rep)
            assert want["run_touch"][0] == n and (n < 255 or 0 < want["run_span"][0] < n and 0 < want["run_inside"][0] < n), (n, column)
            assert (cols[1 if column == "q" else 4] == 1).sum() == n and want["run_touch"][3] == 3


def _mistake_case(name):
    """-> (kwargs for the model on a named case, the case's name)"""
    cols, rep = lattice_case()
    lens = cols[0]
    off, cov = synthetic_coverage(lens, 50)
    covered = dict(threshold=20, cov_offset=off, cov=cov, reso=50)
    if name in ("span_strict", "inside_strict", "self_target_counted", "empty_run_counted"):
        return (cols, False, rep, {}), "lattice_case"
    if name == "target_under_symmetric":
        return (cols, True, rep, {}), "lattice_case, symmetric"
    if name in ("j1_floor", "no_clip_to_W"):                         # runs ending off a window edge; a run ending behind its read
        return (cols, False, rep, covered), "lattice_case with coverage"
    return ([lens[:1]] + [None] * 6, False, csr([[(3990, 3995), (4100, 4200), (-30, -10)]]), dict(covered, cov_offset=off[:2], cov=cov[:off[1]] + 1)), \
        "runs behind and before the read's windows"


@pytest.mark.parametrize("mistake", MISTAKES)
def test_a_planted_mistake_is_caught(mistake):
    (cols, sym, rep, kw), what = _mistake_case(mistake)
    good = repeat_stats_model(*cols, sym, *rep, **kw)
    bad = repeat_stats_model(*cols, sym, *rep, mistake=mistake, **kw)
    same_stats(good, good, what)
    with pytest.raises(AssertionError):
        same_stats(bad, good, f"{what}, with {mistake}")


def test_the_run_behind_the_windows_has_none():
    (cols, sym, rep, kw), _ = _mistake_case("max_of_nothing")
    w = repeat_stats_model(*cols, sym, *rep, **kw)
    assert list(w["run_windows"]) == [1, 0, 0] and list(w["run_cov_max"][1:]) == [0, 0] and w["run_cov_min"][0] > 0
    assert where_of(w["run_flags"]) == ["interior", "tail", "head"]
