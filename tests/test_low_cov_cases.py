"""CPU: the case list of tests/test_gpu_low_cov.py, built from the structural constants of raft_amd/csrc/low_cov.hpp (read back from the
header), the numpy restatement of the low-coverage runs (want_low) beside a plain window-by-window loop, and a census taken from the
cases alone: a run must begin behind, end before and cross every unit boundary the kernels have -- the lane group of each width, the
64-window bitmap word, the tile of low_mark_kernel and the tile of the bitmap kernels -- and every class of read shape must be there.
No grid of low_cov.hpp is capped (every workgroup has a fixed tile), so there is no grid-stride class."""
import os
import re

import numpy as np
from raft_testlib import ROOT, oracle_run

from raft_amd.params import RaftParams

RESO = 50
SHORT = 7                         # bases the last window of every read lacks: len % reso != 0
INTERIOR, HEAD, TAIL, UNCOVERED = 1, 2, 4, 8
RUN_CAP_DELTAS = (-1, 0, 1)       # run_cap one below, equal to and one above n_runs (tests/test_gpu_low_cov.py)


def constants():
    """The structural constants of low_cov.hpp: windows per lane group by output width (4: int32, also what delta4 is decoded
    into; 2; 1), windows per bitmap word, windows per workgroup of low_mark_kernel by width and of the bitmap kernels."""
    text = open(os.path.join(ROOT, "raft_amd", "csrc", "low_cov.hpp")).read()
    bits = open(os.path.join(ROOT, "raft_amd", "csrc", "low_cov_bits.hpp")).read()
    k = {name: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
         for name in ("kLowThreads", "kLowInFlight", "kLowTileWords", "kLowPrefixThreads")}
    k["word"] = int(re.search(r"constexpr int kLowWordWindows = (\d+);", bits).group(1))
    vecs = {t: int(v) for t, v in re.findall(r"struct LowIn<(\w+)> \{ static constexpr int vecs = (\d+);", text)}
    k["lane_windows"] = {4: vecs["int32_t"] * 16 // 4, 2: vecs["uint16_t"] * 16 // 2, 1: vecs["uint8_t"] * 16}
    k["mark_tile"] = {w: k["kLowThreads"] * k["kLowInFlight"] * lw for w, lw in k["lane_windows"].items()}
    k["tile"] = k["kLowTileWords"] * k["word"]
    assert re.search(r"constexpr int kLowMarkGroups = kLowThreads \* kLowInFlight;", text)
    assert not re.search(r"MaxBlocks", text), "a capped grid needs a case larger than one grid step"
    return k


def units(k=None):
    """Every distinct unit boundary, ascending."""
    k = k or constants()
    return sorted(set(k["lane_windows"].values()) | {k["word"], k["tile"]} | set(k["mark_tile"].values()))


# ---- the definition ---------------------------------------------------------------------------------------------------------------------

def want_low(want, read_len, reso, low_cov, permille):
    """The outputs of raft_hip_low_coverage from the oracle's cov / cov_offset, in integer arithmetic."""
    cov = np.asarray(want["cov"], np.int64)
    off = np.asarray(want["cov_offset"], np.int64)
    rl = np.asarray(read_len, np.int64)
    n = off.size - 1
    W = np.diff(off)
    low = cov <= low_cov
    first_of_read = np.zeros(cov.size + 1, bool)
    first_of_read[off[:-1][W > 0]] = True
    first_of_read[cov.size] = True
    before = np.concatenate([[False], low[:-1]])
    after = np.concatenate([low[1:], [False]])
    first = np.flatnonzero(low & (~before | first_of_read[:-1]))
    last = np.flatnonzero(low & (~after | first_of_read[1:]))
    assert first.size == last.size
    read = np.searchsorted(off, first, side="right") - 1          # the largest r with off[r] <= w
    assert np.array_equal(read, np.searchsorted(off, last, side="right") - 1)
    j1, j2 = first - off[read], last - off[read]
    low_s = j1 * reso
    low_e = np.minimum((j2 + 1) * reso, rl[read])
    cls = np.where(j1 == 0, HEAD, 0) | np.where(j2 == W[read] - 1, TAIL, 0) | np.where((j1 > 0) & (j2 < W[read] - 1), INTERIOR, 0)
    flags = np.zeros(n, np.int64)
    np.bitwise_or.at(flags, read, cls)
    low_windows = np.bincount(read, weights=j2 - j1 + 1, minlength=n).astype(np.int64)[:n] if n else np.zeros(0, np.int64)
    low_bases = np.bincount(read, weights=low_e - low_s, minlength=n).astype(np.int64)[:n] if n else np.zeros(0, np.int64)
    flags |= np.where(1000 * low_bases > permille * rl, UNCOVERED, 0)
    return {"low_offset": np.searchsorted(read, np.arange(n + 1), side="left").astype(np.int64), "low_s": low_s.astype(np.int32),
            "low_e": low_e.astype(np.int32), "low_windows": low_windows.astype(np.int32), "low_flags": flags.astype(np.uint8),
            "n_runs": int(first.size), "total_low_windows": int(low_windows.sum()), "low_bases": int(low_bases.sum()),
            "reads_with_runs": int((low_windows > 0).sum()), "reads_interior": int(((flags & INTERIOR) != 0).sum()),
            "reads_uncovered": int(((flags & UNCOVERED) != 0).sum())}


def want_low_slow(want, read_len, reso, low_cov, permille):
    """The same, one window at a time."""
    cov, off = want["cov"], want["cov_offset"]
    out = {"low_offset": [0], "low_s": [], "low_e": [], "low_windows": [], "low_flags": []}
    bases_all = 0
    for r in range(len(off) - 1):
        W = int(off[r + 1] - off[r])
        L = int(read_len[r])
        j, nwin, bases, f = 0, 0, 0, 0
        while j < W:
            if cov[off[r] + j] > low_cov:
                j += 1
                continue
            j1 = j
            while j < W and cov[off[r] + j] <= low_cov:
                j += 1
            j2 = j - 1
            s, e = j1 * reso, min((j2 + 1) * reso, L)
            out["low_s"].append(s); out["low_e"].append(e)
            nwin += j2 - j1 + 1; bases += e - s
            f |= (HEAD if j1 == 0 else 0) | (TAIL if j2 == W - 1 else 0) | (INTERIOR if j1 > 0 and j2 < W - 1 else 0)
        if 1000 * bases > permille * L:
            f |= UNCOVERED
        bases_all += bases
        out["low_offset"].append(len(out["low_s"])); out["low_windows"].append(nwin); out["low_flags"].append(f)
    res = {k: np.asarray(v, {"low_offset": np.int64, "low_flags": np.uint8}.get(k, np.int32)) for k, v in out.items()}
    fl = res["low_flags"]
    res.update(n_runs=len(out["low_s"]), total_low_windows=int(sum(out["low_windows"])), low_bases=bases_all,
               reads_with_runs=int((res["low_windows"] > 0).sum()), reads_interior=int(((fl & INTERIOR) != 0).sum()),
               reads_uncovered=int(((fl & UNCOVERED) != 0).sum()))
    return res


def same_low(got, exp, what):
    for k in ("low_offset", "low_s", "low_e", "low_windows", "low_flags"):
        assert got[k].dtype == exp[k].dtype and got[k].shape == exp[k].shape, (what, k, got[k].dtype, got[k].shape, exp[k].shape)
        bad = np.flatnonzero(got[k] != exp[k])
        assert bad.size == 0, f"{what}: {k} differs in {bad.size} places, first at {bad[0]}: got {got[k][bad[0]]} want {exp[k][bad[0]]}"
    for k in ("n_runs", "total_low_windows", "low_bases", "reads_with_runs", "reads_interior", "reads_uncovered"):
        assert got[k] == exp[k], (what, k, got[k], exp[k])


# ---- inputs with a chosen coverage ------------------------------------------------------------------------------------------------------

def cover(windows, depth, reso=RESO, short=SHORT):
    """Reads of the given window counts (0: a read of length 0; otherwise the last window lacks `short` bases) and self overlaps under
    which window w of the concatenated array has coverage depth[w]: per level d, one record (r, j1 * reso, min((j2 + 1) * reso, len))
    for every maximal stretch j1..j2 of windows of read r with depth >= d.  For symmetric_mode = 1."""
    W = np.asarray(windows, np.int64)
    depth = np.asarray(depth, np.int64)
    off = np.concatenate([[0], np.cumsum(W)])
    assert depth.size == off[-1]
    rl = np.where(W > 0, W * reso - short, 0).astype(np.int32)
    first_of_read = np.zeros(depth.size + 1, bool)
    first_of_read[off[:-1][W > 0]] = True
    first_of_read[depth.size] = True
    qid, qs, qe = [], [], []
    for d in range(1, int(depth.max(initial=0)) + 1):
        m = depth >= d
        a = np.flatnonzero(m & (~np.concatenate([[False], m[:-1]]) | first_of_read[:-1]))
        b = np.flatnonzero(m & (~np.concatenate([m[1:], [False]]) | first_of_read[1:]))
        r = np.searchsorted(off, a, side="right") - 1
        qid.append(r); qs.append((a - off[r]) * reso); qe.append(np.minimum((b - off[r] + 1) * reso, rl[r]))
    cat = lambda xs: np.concatenate(xs).astype(np.int32) if xs else np.empty(0, np.int32)
    qid, qs, qe = cat(qid), cat(qs), cat(qe)
    return [rl, qid, qs, qe, qid.copy(), qs.copy(), qe.copy()]


def _flat(n, low, value=1):
    d = np.full(n, value, np.int64)
    for a, b in low:
        d[a:b + 1] = 0
    return d


def low_cases():
    """name -> (windows of every read, coverage of every window)."""
    k = constants()
    T = k["tile"]
    cases = {}
    for U in units(k):
        P = U if U >= k["word"] else 3 * U
        n = P + min(U, 40) + 5
        cases[f"begins_after_{U}"] = ([n], _flat(n, [(P, P + 2)]))
        cases[f"ends_before_{U}"] = ([n], _flat(n, [(P - 3, P - 1)]))
        cases[f"crosses_{U}"] = ([n], _flat(n, [(P - 2, P + 1)]))
        cases[f"read_boundary_on_{U}"] = ([P, n - P], _flat(n, [(P - 2, P + 1)]))
    n = 2 * T + 300
    cases["crosses_two_tiles"] = ([n], _flat(n, [(T - 100, 2 * T + 100)]))
    cases["read_boundary_inside_a_lane_group"] = ([13, 14], _flat(27, [(10, 16)]))
    ones = 150
    d = _flat(10 + ones, [(3, 4)])
    d[5:5 + ones] = (np.arange(ones) % 3 == 0)                      # one-window reads, two of three low
    cases["one_window_reads"] = ([5] + [1] * ones + [5], d)
    cases["empty_reads_between_two_low_reads"] = ([6, 0, 0, 7], _flat(13, [(4, 7)]))
    cases["a_read_of_one_low_window"] = ([1], _flat(1, [(0, 0)]))
    cases["a_read_of_one_covered_window"] = ([1], _flat(1, []))
    n = T + 203
    cases["every_other_window"] = ([n], (np.arange(n) % 2).astype(np.int64))
    cases["all_low"] = ([100, 37], _flat(137, [(0, 136)]))
    cases["none_low"] = ([100, 37], _flat(137, []))
    cases["no_windows"] = ([0, 0, 0], _flat(0, []))
    for r in range(16):                                             # n_bins = 32 + r: every residue modulo 16, tails shorter than a lane group
        n = 32 + r
        cases[f"residue_{r}"] = ([20, 12 + r], _flat(n, [(18, 21), (n - 3, n - 1)]))
    cases["stacked_depths"] = ([200, 90, 3], (np.arange(293) // 5) % 4)        # depths 0..3 in stretches of five
    cases["head_interior_tail"] = ([40, 40, 40], _flat(120, [(0, 3), (10, 12), (36, 39), (50, 60), (110, 119)]))
    return cases


# ---- the census -------------------------------------------------------------------------------------------------------------------------

def census(windows, depth, k, low_cov=0):
    """The classes of one case, from its window counts and coverage alone."""
    W = np.asarray(windows, np.int64)
    off = np.concatenate([[0], np.cumsum(W)])
    n_bins = int(off[-1])
    if n_bins == 0:
        return {"no_windows"}
    T = k["tile"]
    low = np.asarray(depth) <= low_cov
    out = {f"residue_{n_bins % 16}"}
    if 0 < n_bins % 16 < min(k["lane_windows"].values()):
        out.add("tail_shorter_than_a_lane_group")
    out.add("all_low" if low.all() else "none_low" if not low.any() else "some_low")
    # runs, by the definition: a read at a time
    runs = []
    for r in range(W.size):
        j = int(off[r])
        while j < off[r + 1]:
            if not low[j]:
                j += 1
                continue
            a = j
            while j < off[r + 1] and low[j]:
                j += 1
            runs.append((a, j - 1, r))
    inner = [b for b in off[1:-1] if 0 < b < n_bins]
    for U in units(k):
        for a, b, r in runs:
            if a > 0 and a % U == 0 and not low[a - 1] and a > off[r]:
                out.add(f"begins_after_{U}")
            if b % U == U - 1 and b + 1 < off[r + 1] and not low[b + 1]:
                out.add(f"ends_before_{U}")
            if a // U < b // U:
                out.add(f"crosses_{U}")
        if any(b % U == 0 and low[b - 1] and low[b] for b in inner):
            out.add(f"read_boundary_on_{U}")
    if any(b // T - a // T >= 2 for a, b, _ in runs):
        out.add("crosses_two_tiles")
    if any(b % max(k["lane_windows"].values()) not in (0, min(k["lane_windows"].values())) and low[b - 1] and low[b] for b in inner):
        out.add("read_boundary_inside_a_lane_group")
    one = np.concatenate([[0], (W == 1).astype(np.int8), [0]])
    edges = np.flatnonzero(np.diff(one))
    for a, b in zip(edges[::2], edges[1::2]):
        seg = low[off[a]:off[b]]
        if b - a > k["word"] and seg.any() and not seg.all():
            out.add("one_window_reads_in_a_row_longer_than_a_word")
    nz = np.flatnonzero(W > 0)
    for x, y in zip(nz[:-1], nz[1:]):
        if y - x > 1 and low[off[x + 1] - 1] and low[off[y]]:
            out.add("empty_reads_between_two_low_reads")
    if (W == 1).any():
        out.add("a_read_of_one_window")
    alt = np.flatnonzero(np.concatenate([[True], low[1:] == low[:-1], [True]]))      # stretches in which neighbours always differ
    if np.diff(alt).max() > T:
        out.add("every_other_window_over_more_than_a_tile")
    if any(b == off[r + 1] - 1 for a, b, r in runs) and SHORT % RESO != 0:
        out.add("a_run_reaches_a_partial_last_window")
    return out


def required(k):
    need = {f"residue_{r}" for r in range(16)} | {
        "tail_shorter_than_a_lane_group", "all_low", "none_low", "some_low", "no_windows", "crosses_two_tiles", "read_boundary_inside_a_lane_group",
        "one_window_reads_in_a_row_longer_than_a_word", "empty_reads_between_two_low_reads", "a_read_of_one_window",
        "every_other_window_over_more_than_a_tile", "a_run_reaches_a_partial_last_window"}
    for U in units(k):
        need |= {f"begins_after_{U}", f"ends_before_{U}", f"crosses_{U}", f"read_boundary_on_{U}"}
    return need


# ---- tests ------------------------------------------------------------------------------------------------------------------------------

def test_constants_are_what_the_cases_assume():
    k = constants()
    assert k["lane_windows"] == {4: 8, 2: 8, 1: 16} and k["word"] == 64
    assert k["kLowTileWords"] == k["kLowThreads"]
    assert all(k["tile"] % m == 0 for m in k["mark_tile"].values())
    assert RUN_CAP_DELTAS == (-1, 0, 1)


def test_every_class_is_present():
    k = constants()
    seen = set()
    for name, (windows, depth) in low_cases().items():
        seen |= census(windows, depth, k)
    assert not (required(k) - seen), sorted(required(k) - seen)


def test_cover_gives_the_coverage_and_want_low_the_class():
    """The oracle's cov[] of every case is the chosen one, want_low equals the window-by-window loop on it, and what it yields is the
    class the census claims for the case's name."""
    k = constants()
    p = RaftParams(est_cov=30, symmetric_mode=1)
    for name, (windows, depth) in low_cases().items():
        cols = cover(windows, depth)
        want = oracle_run(p, *cols)
        assert np.array_equal(want["cov"], depth), name
        assert np.array_equal(np.diff(want["cov_offset"]), windows), name
        for low_cov in (0, 1, 2) if name == "stacked_depths" else (0,):
            fast = want_low(want, cols[0], RESO, low_cov, 800)
            same_low(fast, want_low_slow(want, cols[0], RESO, low_cov, 800), f"{name}, low_cov {low_cov}")
        w = want_low(want, cols[0], RESO, 0, 800)
        cls = census(windows, depth, k)
        assert name in cls or name in ("one_window_reads", "a_read_of_one_low_window", "a_read_of_one_covered_window", "every_other_window",
                                       "stacked_depths", "head_interior_tail"), (name, sorted(cls))
        if name.startswith("read_boundary_on_") or name == "read_boundary_inside_a_lane_group":
            assert w["n_runs"] == 2 and list(w["low_flags"] & 7) == [TAIL, HEAD], name            # two runs, not one
        if name.startswith(("begins_after_", "ends_before_", "crosses_")):
            assert w["n_runs"] == 1 and w["low_flags"][0] & 7 == INTERIOR, name
        if name == "all_low":
            assert list(w["low_flags"]) == [HEAD | TAIL | UNCOVERED] * 2 and list(w["low_e"]) == [100 * RESO - SHORT, 37 * RESO - SHORT]
        if name == "none_low":
            assert w["n_runs"] == 0 and not w["low_flags"].any()
        if name == "every_other_window":
            assert w["n_runs"] == (windows[0] + 1) // 2 == (sum(windows) + len(windows)) // 2      # the bound of raft_hip.h is reached
        if name == "empty_reads_between_two_low_reads":
            assert list(w["low_offset"]) == [0, 1, 1, 1, 2]
        if name == "head_interior_tail":
            assert list(w["low_flags"] & 7) == [HEAD | INTERIOR | TAIL, INTERIOR, TAIL]
        assert w["n_runs"] <= (sum(windows) + len(windows)) // 2
