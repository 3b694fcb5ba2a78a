"""CPU: the lattice sets of raft_testlib (runs of high windows placed on every lane / half-row / row / tile / piece boundary of the
wave kernel's geometry, values on either side of every threshold) against the oracle -- and the census that keeps them honest.

For every set: the oracle's cov, rep_offset, rep_s, rep_e equal the generator's closed form (every read of every set is compared),
and, from the oracle's output alone, every boundary class holds at least one run that ENDS on its last window and one that BEGINS
on its first, one window short of repeat_length and exactly long enough.  tests/test_gpu_lattice.py runs the same sets through both
pileup kernels, every input form and every encoding; what this file establishes is that those runs are aimed where they claim to be.
Where the compiled reference is built (oracle/_ref), `rows` and `pieces` go through it as well.
"""
import numpy as np
import pytest
import raft_testlib as T
from raft_testlib import (D4_BLOCK, DEPTH_NS, STEP_KS, TILE_CAP, assert_lattice_result, have_ref_lib, lattice_byte_level, lattice_census,
                          lattice_depth, lattice_first_difference, lattice_pieces, lattice_rows, lattice_steps, lattice_tile_end, ref_lib_run)

ROW_CLASSES = [(nm, x, side, d) for nm in ("lane", "half-row", "row") for x in range(4) for side in ("end", "begin") for d in (-1, 0)]


def check_closed_form(case, want):
    """The oracle against the construction: coverage of every window, the repeats of every read."""
    ex = case.expect
    assert np.array_equal(want["cov_offset"], ex["cov_offset"]), case.name
    msg = lattice_first_difference(case, want, ex)
    assert msg is None, f"set {case.name}, oracle against the closed form: {msg}"
    assert want["high_cov"] == case.p.high_cov


def require(census, keys, name):
    missing = [k for k in keys if census.get(k, 0) < 1]
    assert not missing, f"set {name}: no run on {len(missing)} boundary classes (class, alignment, side, d): {missing[:12]}"


@pytest.mark.parametrize("which", ["r50", "r7", "flank", "h1"])
def test_rows_and_threshold(which):
    case = lattice_rows(which)
    want = case.oracle()
    check_closed_form(case, want)
    census = lattice_census(case, want)
    require(census, ROW_CLASSES, case.name)
    # the sets hold what they say: both kinds of read in numbers, every alignment of a read's offset, partial last windows
    n_rep = np.diff(want["rep_offset"])
    run = np.array([k == "run" for k in case.kind])
    assert np.all(n_rep[run & (case.d == -1)] == 0) and np.all(n_rep[run & (case.d >= 0)] == 1)
    assert np.all(n_rep[np.array([k == "two" for k in case.kind]) & (case.d >= 0)] == 2)
    assert set((want["cov_offset"][:-1] % 4).tolist()) == {0, 1, 2, 3}
    assert set((case.cols[0] % case.p.reso).tolist()) >= {0, 1, case.p.reso - 1}
    if which == "flank":       # the flank reaches beyond both ends of every read
        r = np.repeat(np.arange(case.n_reads), n_rep)
        assert np.all(want["rep_s"] == 0) and np.array_equal(want["rep_e"], case.cols[0][r])
    if which == "h1":
        assert want["high_cov"] == 1 and set(np.unique(want["cov"]).tolist()) == {0, 1}
    if which in ("r50", "r7") and have_ref_lib():
        ref = ref_lib_run(case.p, *case.cols)
        assert lattice_first_difference(case, ref, want) is None, lattice_first_difference(case, ref, want)


def test_tile_end():
    case = lattice_tile_end()
    want = case.oracle()
    check_closed_form(case, want)
    off, high = want["cov_offset"], want["cov"] >= want["high_cov"]
    W = np.diff(off)
    m = case.p.repeat_length // case.p.reso
    last_high = high[off[1:] - 1] & ~high[off[1:] - 2 - m]              # a run that ends on the read's last window, shorter than m + 2
    for k in range(-8, 9):                                              # around the cap: the sentinel slot, the first windows of a second piece
        for d in (-1, 0):
            sel = (W == TILE_CAP - k) & last_high & (case.d == d) & np.array([kd == "end-0" for kd in case.kind])
            assert sel.sum() >= 1, (k, d)
    assert W.min() <= TILE_CAP - 512 and W.max() >= TILE_CAP + 8       # a row below, pieces above
    assert np.all(W > TILE_CAP // 2)                                    # one read per tile
    assert set((off[:-1] % 4).tolist()) == {0, 1, 2, 3}


def test_pieces():
    case = lattice_pieces()
    want = case.oracle()
    check_closed_form(case, want)
    census = lattice_census(case, want)
    require(census, [("piece", -1, side, d) for side in ("end", "begin") for d in (-1, 0)], case.name)
    # the short run straddles a piece edge in every split; a piece high from end to end; runs longer than a piece
    off, cov = want["cov_offset"], want["cov"]
    m = case.p.repeat_length // case.p.reso
    run = np.array([k == "run" for k in case.kind])
    for edge in (TILE_CAP, 2 * TILE_CAP):
        for d in (-1, 0):
            for left in range(1, m + d):
                a = edge - left - (edge - TILE_CAP)                     # (the second run of a read lies TILE_CAP behind its first)
                assert np.any(run & (case.a == a) & (case.d == d)), (edge, d, left)
    high = cov >= want["high_cov"]
    whole = [r for r in range(case.n_reads) if case.W[r] >= 2 * TILE_CAP and high[off[r] + TILE_CAP: off[r] + 2 * TILE_CAP].all()]
    assert len(whole) >= 3
    assert {int(case.d[r]) + m for r in range(case.n_reads) if case.kind[r].startswith("long")} == {TILE_CAP - 1, TILE_CAP, TILE_CAP + 1, 2 * TILE_CAP}
    assert case.W.max() < 65535                                         # (window records hold 16 bits)
    if have_ref_lib():
        ref = ref_lib_run(case.p, *case.cols)
        assert lattice_first_difference(case, ref, want) is None, lattice_first_difference(case, ref, want)


def test_byte_level():
    case = lattice_byte_level()
    want = case.oracle()
    check_closed_form(case, want)
    require(lattice_census(case, want), ROW_CLASSES, case.name)
    cov, off = want["cov"], want["cov_offset"]
    assert set(np.unique(cov).tolist()) == {254, 255, 256}
    r = np.searchsorted(off, np.arange(cov.size), side="right") - 1
    slot = np.arange(cov.size) - off[r] + off[r] % 4
    for v in (255, 256):                                                # both escaped values on both sides of every boundary kind
        for B in (4, 256, 512):
            assert np.any((cov == v) & (slot % B == B - 1)) and np.any((cov == v) & (slot % B == 0)), (v, B)


def test_steps():
    case = lattice_steps()
    want = case.oracle()
    check_closed_form(case, want)
    cov, off = want["cov"].astype(np.int64), want["cov_offset"]
    step = np.diff(np.concatenate([[0], cov]))
    g = np.arange(cov.size)
    assert set(np.unique(np.abs(step[step != 0])).tolist()) == set(STEP_KS)
    for k in (7, 8):                                                    # fits / is listed, up and down, on every residue of the anchor blocks
        for s in (k, -k):
            assert np.unique(g[step == s] % D4_BLOCK).size == D4_BLOCK, (s,)
    for k in STEP_KS:
        for s in (k, -k):
            res = set((g[step == s] % D4_BLOCK).tolist())
            assert {0, 1, D4_BLOCK - 1} <= res, (s,)
        assert np.any(step[off[:-1]] == k)                               # a = 0 of a read
    require(lattice_census(case, want), [("block", -1, side, d) for side in ("end", "begin") for d in (-1, 0)], case.name)
    # high_cov = 8: coverage high_cov - 1 and high_cov side by side in one set
    n_rep = np.diff(want["rep_offset"])
    kk = np.array([int(s.split("=")[1].split(" ")[0]) for s in case.kind])
    assert np.all(n_rep[kk < 8] == 0) and np.all(n_rep[(kk >= 8) & (case.d >= 0)] == 1) and np.all(n_rep[case.d < 0] == 0)


@pytest.mark.parametrize("H", [3, 32767, 32768, 65537])
def test_depth(H):
    case = lattice_depth(H)
    want = case.oracle()
    check_closed_form(case, want)
    off = want["cov_offset"]
    n_rec = np.bincount(case.cols[1], minlength=case.n_reads)
    starts, ends = set(), set()
    for r in range(case.n_reads):
        if case.kind[r].startswith("N="):
            N = int(case.kind[r][2:])
            assert n_rec[r] == N and want["cov"][off[r]:off[r + 1]].max() == N      # the read's record count IS its deepest window
            assert case.W[r] > TILE_CAP // 2
            hot = np.flatnonzero(want["cov"][off[r]:off[r + 1]] >= N - 30)
            starts.add(int(hot[0] + off[r] % 4) % 2); ends.add(int(hot[-1] + off[r] % 4) % 2)
        else:
            assert case.W[r] > TILE_CAP // 2 and n_rec[r] == 3
    assert starts == {0, 1} and ends == {0, 1}                                       # both halves of an LDS dword
    assert sorted(int(k[2:]) for k in case.kind if k.startswith("N=")) == list(DEPTH_NS)
    assert want["high_cov"] == H
    deep = np.array([k.startswith("N=") for k in case.kind])
    n_rep = np.diff(want["rep_offset"])
    if H == 3:
        assert np.all(n_rep[deep] == 1)
    else:                                     # a run of high windows only where N reaches the threshold; never long enough beyond 3
        assert np.all(n_rep == 0)
        n_high = np.add.reduceat((want["cov"] >= H).astype(np.int64), off[:-1])
        assert np.array_equal(n_high[deep] > 0, np.array([int(k[2:]) for k in case.kind if k.startswith("N=")]) >= H)
    small = lattice_depth(H, Ns=tuple(n for n in DEPTH_NS if n <= 32767))
    check_closed_form(small, small.oracle())
    assert np.bincount(small.cols[1]).max() == 32767


def test_a_wrong_result_is_named_by_its_coordinate():
    """The checks can fail, and say where: a repeat shifted by one window, a coverage value truncated to 16 bits."""
    case = lattice_rows("r50")
    want = case.oracle()
    r = int(np.flatnonzero((case.a == 507) & (case.d == 0) & np.array([k == "run" for k in case.kind]))[0])
    bad = dict(want, rep_e=want["rep_e"].copy())
    bad["rep_e"][want["rep_offset"][r]] += case.p.reso
    with pytest.raises(AssertionError) as e:
        assert_lattice_result(case, bad, want, "columns, wave kernel, width 4")
    msg = str(e.value)
    assert "set rows/reso 50, columns, wave kernel, width 4" in msg and f"read {r} [run] (a=507, d=0, W={int(case.W[r])}, offset mod 4={int(want['cov_offset'][r] % 4)})" in msg
    bad = dict(want, cov=want["cov"].copy())
    bad["cov"][want["cov_offset"][r] + 507] -= 1
    with pytest.raises(AssertionError) as e:
        assert_lattice_result(case, bad, want, "w")
    assert "(a=507, d=0" in str(e.value) and "at window 507" in str(e.value)
    # the closed form is no echo of the oracle: the same shift in the construction is caught by check_closed_form
    shifted = T.LatticeCase(case.name, case.p, case.cols, dict(case.expect, rep_s=case.expect["rep_s"] + 0), case.a, case.d, case.W, case.kind)
    shifted.expect["rep_s"][want["rep_offset"][r]] += case.p.reso
    with pytest.raises(AssertionError, match="a=507, d=0"):
        check_closed_form(shifted, want)
    deep = lattice_depth(3)
    dw = deep.oracle()
    cut = dict(dw, cov=dw["cov"] & 0xFFFF)
    with pytest.raises(AssertionError) as e:
        assert_lattice_result(deep, cut, dw, "windows, deep kernel, width 2")
    assert "[N=65536]" in str(e.value) and "got 0 want 65536" in str(e.value)
