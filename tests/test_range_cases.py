"""CPU: the range sets of tests/range_cases.py (reads, records and runs of high windows on the boundaries at which the ranges of the
pileup kernel's hand-out begin) against the oracle -- and what keeps them honest.

Every set equals the oracle read by read (coverage, repeats: the closed form is the construction's).  A census made from the
ORACLE's output and the reads' cov_offset counts the reads of every class the layout's plan names -- (kind of boundary, -1 / 0 / +1),
reads of one and of no window on a boundary, reads ending on at(k) - 1 and at(k), runs across a boundary one window short and
long enough, ranges and shares in which no read begins -- and fails on an empty class; which classes a set must fill follows from
its geometry, worked out here.  The constants the sets are laid on are read back from the sources.  tests/test_quantum.py pins the
boundaries themselves to raft_amd/csrc/quantum.hpp; tests/test_gpu_ranges.py runs the sets through the engine."""
import os
import re

import numpy as np
import pytest
import range_cases as R
from raft_testlib import ROOT, TILE_CAP, assert_lattice_result

CSRC = os.path.join(ROOT, "raft_amd", "csrc")
FULL = [B for B in R.GRADED_BS if B >= 200_000]


def test_the_constants_the_sets_are_built_on():
    eng, qh, ctx, wl, wlh, wave = (open(os.path.join(CSRC, f)).read() for f in
                                   ("engine.hip", "quantum.hpp", "engine_ctx.hpp", "wave_launch.hpp", "wave_launch.hip", "pileup_wave.hpp"))

    def one(pattern, text):
        m = re.findall(pattern, text)
        assert len(m) == 1, (pattern, m)
        return m[0]
    assert int(one(r"#define RAFT_WAVE_SLOTS (\d+)\b", wl)) - int(one(r"constexpr int kTileCap = kWaveSlots - (\d+);", ctx)) == TILE_CAP
    assert one(r"q1 = \(kTileCap / (\d+)\) \* (\d+);", eng) == ("128", "128") and R.Q1 == TILE_CAP // 128 * 128 == 3968
    assert one(r"graded_quantum\(B, (\d+) \* \(int\)q1, (\d+) \* \(int\)q1, ([0-9.]+)\)", eng) == ("8", "2", "0.9")
    assert (R.Q_LONG, R.Q_SHORT, R.FRAC_LONG) == (8 * R.Q1, 2 * R.Q1, 0.9) == (31744, 7936, 0.9)
    assert one(r"z\.share = \(\(n_windows \+ 7\) / (\d+) \+ (\d+)\) / (\d+) \* (\d+);", qh) == ("8", "127", "128", "128") and R.ROUND == 128
    assert int(one(r"sw\.graded_min >= 0 \? sw\.graded_min : (\d+)LL \* wave_grid_waves\(true\);", eng)) * R.WORKERS == R.GRADED_MIN_DEFAULT
    one(r"B / kTileCap >= graded_min && \(B \+ 7\) / 8 \+ 128 < \(1LL << 31\)", eng)
    assert int(one(r"\n    int n_ctr = (\d+);", eng)) == R.COUNTERS == 8
    one(r"share_q = \(int\)\(\(unsigned\)n_seg_tiles / \(unsigned\)kCtr\), share_r = n_seg_tiles - share_q \* kCtr;", wave)
    one(r"const int d0 = ctr \* share_q \+ min\(ctr, share_r\), d1 = d0 \+ share_q \+ \(ctr < share_r \? 1 : 0\);", wave)
    assert one(r"int wave_grid_waves\(bool win\) \{ return (\d+) \* (\d+) \* \(win \? kWpsWin : kWpsCols\); \}", wlh) == ("256", "4")
    assert 256 * 4 * int(one(r"#define RAFT_WAVE_WPS (\d+) ", wl)) == R.WORKERS == 4096
    one(r"#define RAFT_WAVE_WPS_COLS RAFT_WAVE_WPS\n", wlh)
    one(r"const int Q = c->tile_q \? std::max\(256, c->tile_q\)", eng)
    assert R.UNIFORM_Q == 256
    # the thresholds the issue names
    assert R.graded_geometry(100) == (128, 0, 1) and R.graded_geometry(281_600)[1] == 0 and R.graded_geometry(281_601)[1] == 1
    assert R.GRADED_MIN_DEFAULT * TILE_CAP == 1_072_693_248
    assert 8 * R.graded_geometry(5_840_896)[2] == 256 and 8 * R.graded_geometry(5_900_000)[2] > 256


def require(census, keys, what):
    missing = [k for k in keys if census.get(k, 0) < 1]
    assert not missing, f"{what}: no read in the classes {missing}"


def show(what, census):
    print(f"census {what}: " + ", ".join(f"{' '.join(str(x) for x in k)} = {v}" for k, v in sorted(census.items(), key=str) if v))


def check_closed_form(case, want):
    for k in ("cov_offset", "cov", "rep_offset", "rep_s", "rep_e"):
        g, w = case.expect[k], want[k]
        assert g.shape == w.shape, (case.name, k, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        if bad.size:
            off = want["cov_offset"] if k.startswith("cov") else want["rep_offset"]
            r = int(np.searchsorted(off, bad[0], side="right") - 1) if not k.endswith("offset") else int(bad[0]) - 1
            raise AssertionError(f"oracle against the closed form: {k} differs first in set {case.name}, {case.coordinate(max(r, 0))}")
    assert want["high_cov"] == R.HIGH and want["total_windows"] == case.B
    # records exist for the reads on either side of every boundary: every read with a window has one
    n_rec = np.bincount(case.cols[1], minlength=case.n_reads)
    assert np.all((n_rec >= 1) == (case.W > 0))


@pytest.mark.parametrize("B", R.GRADED_BS)
def test_graded(B, capsys):
    case = R.ranges_graded(B)
    want = case.oracle()
    check_closed_form(case, want)
    census = R.range_census(case, want)
    share, n_long, per_share = R.graded_geometry(B)
    keys = R.census_wanted(case)
    placed = {(kind, what) for kind, what, _ in case.plan}
    if B in FULL:
        # what the geometry has, the plan must have placed: every pattern at every kind of boundary, "starts" on the set's last one
        kinds = {"share", "short-short"} | ({"long-long", "long-short"} if n_long >= 2 else set()) | \
                ({"closing"} if (share - n_long * R.Q_LONG) % R.Q_SHORT else set())
        assert {k for k in case.kinds} == kinds, (B, kinds)
        assert placed >= {(kind, pattern) for kind in kinds for pattern in R.PATTERNS} | {("last", "starts")}, sorted(placed, key=str)
        assert ("share", "more than a tile's windows, straddles a share's end") in placed
        if n_long >= 4:
            assert ("long-long", "reaches over two boundaries of the long part") in placed
        assert np.sum(case.W > TILE_CAP) >= 1
    if B >= 5_000_000:
        assert ("short-short", "reaches over nine boundaries of the short part") in placed and len(case.kinds) > 256
        # tile_desc_kernel looks up a boundary per thread: lane 63 / 64 and the workgroup's edge 255 / 256 are boundaries with reads on them
        assert all(case.at[k] < B and any(abs(int(p) - int(case.at[k])) == 0 for _, _, p in case.plan) for k in (63, 64, 255, 256))
    if B == 5_900_000:
        assert [case.kinds[k] for k in (63, 64, 255, 256)] == ["short-short"] * 4
    if B == 7_200_000:
        assert [case.kinds[k] for k in (63, 64, 255, 256)] == ["long-long", "long-short", "long-long", "long-long"]
    if B == 100:
        assert census.get(("no read begins in a share",), 0) == 7 and placed == {("share", "empty")}
    if B == 129:
        assert census.get(("no read begins in a share",), 0) == 6 and census.get(("share", 0), 0) >= 2
    assert 8 * share - B == {888_832: 0, 888_833: 1023}.get(B, 8 * share - B)           # (nothing and as much as can lie behind the set)
    require(census, keys, case.name)
    assert case.n_reads <= 4000 and case.cols[1].size <= 1.1 * case.n_reads + 16         # (about where reads lie, not about depth)
    with capsys.disabled():
        show(f"{case.name}: share {share}, n_long {n_long}, per_share {per_share}, {case.n_reads} reads", census)


@pytest.mark.parametrize("n_ranges", R.UNIFORM_NS)
def test_uniform(n_ranges, capsys):
    case = R.ranges_uniform(n_ranges)
    want = case.oracle()
    check_closed_form(case, want)
    assert case.B // R.UNIFORM_Q + 1 == n_ranges
    census = R.range_census(case, want)
    require(census, R.census_wanted(case), case.name)
    # every counter with a share has a placement at its first and at its last range (but range 0, which begins the set)
    shares = R.counter_shares(n_ranges)
    assert shares[0][0] == 0 and shares[-1][1] == n_ranges and all(a[1] == b[0] for a, b in zip(shares, shares[1:]))
    placed_at = {p // R.UNIFORM_Q for _, _, p in case.plan}
    ends = {d for d0, d1 in shares if d1 > d0 for d in (d0, d1 - 1)}
    assert placed_at >= ends - ({0} if n_ranges > 1 else set()), (sorted(ends), sorted(placed_at))
    q, r = divmod(n_ranges, R.COUNTERS)
    assert [d1 - d0 for d0, d1 in shares] == [q + 1] * r + [q] * (R.COUNTERS - r)      # (both sides of share_r)
    if n_ranges >= 17:
        assert {what for _, what, _ in case.plan} == set(R.PATTERNS)
    with capsys.disabled():
        show(f"{case.name}: {case.B} windows, {case.n_reads} reads, shares of {q} + {r}", {k: v for k, v in census.items() if "counter" not in str(k[0])})


def test_both_sides_of_share_r_and_of_the_worker_count():
    rs = {n % R.COUNTERS for n in R.UNIFORM_NS}
    assert 0 in rs and len(rs) >= 4
    assert {R.WORKERS - 1, R.WORKERS, R.WORKERS + 1, 8 * R.WORKERS + 3} <= set(R.UNIFORM_NS) and min(R.UNIFORM_NS) == 1
    assert sum(n < R.COUNTERS for n in R.UNIFORM_NS) >= 3


def test_a_wrong_result_is_named_by_its_boundary():
    case = R.ranges_graded(888_833)
    want = case.oracle()
    r = case.kind.index("one window on the boundary")
    w = int(want["cov_offset"][r])
    k = case.idx(w)
    assert case.at[k] == w
    bad = dict(want, cov=want["cov"].copy())
    bad["cov"][w] += 1
    with pytest.raises(AssertionError) as e:
        assert_lattice_result(case, bad, want, "form columns, kernel wave, width 4, pass 1")
    msg = str(e.value)
    assert msg.startswith("set ranges_graded(888833), form columns, kernel wave, width 4, pass 1: cov differs in 1 windows, first in read ")
    assert f"[one window on the boundary] windows [{w}, {w + 1}), begins +0 from boundary k={k} (class {case.kinds[k]}, at {w}) of the graded quantum, B=888833" in msg
    # and the closed form is no echo of the oracle
    with pytest.raises(AssertionError, match=r"\('ranges_graded\(888832\)', 'cov_offset'"):
        check_closed_form(R.ranges_graded(888_832), want)
    other = R.RangeCase(case.name, case.p, case.cols, dict(case.expect, cov=bad["cov"]), case.W, case.kind, case.at, case.kinds, case.plan, case.B, case.quantum)
    with pytest.raises(AssertionError, match=r"oracle against the closed form: cov differs first in set ranges_graded\(888833\), read \d+ \[one window on the boundary\]"):
        check_closed_form(other, want)
