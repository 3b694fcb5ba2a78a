"""CPU: what the sets of tests/line_cases.py hold, taken from the oracle's side -- so that tests/test_gpu_line_aligned.py cannot go
vacuous unnoticed (in the manner of tests/test_lattice_cases.py)."""
import numpy as np
from line_cases import (LINE, M, PLACEMENTS, SLOTS, W_PIECES, census, deep_tile, feasible_classes, in_runs, mixed_tiles, single_read_tiles,
                        w_class)
from raft_testlib import TILE_CAP, oracle_run


def _oracle(p, cols):
    rl, qid, qs, qe = cols
    return oracle_run(p, rl, qid, qs, qe, qid, qs, qe)


def test_single_read_tiles_hold_every_residue_class_and_placement():
    p, cols, cases = single_read_tiles()
    want = _oracle(p, cols)
    off = want["cov_offset"]
    W = np.diff(off)
    assert W.min() >= 2047                                       # no two reads fit one array: every tile is one read or a piece of one
    assert 2 * 2047 > TILE_CAP
    got = census(off, want["cov"], want["high_cov"])
    missing = [(al, c, pl) for al in range(LINE) for c in feasible_classes(al) for pl in PLACEMENTS if got.get((al, c, pl), 0) < 1]
    assert not missing, f"{len(missing)} empty classes (residue, W class, placement): {missing[:12]}"
    # the three sums next to the array's end exist wherever a read of up to TILE_CAP windows can reach them
    case_r = np.array([c[0] for c in cases])
    s = off[case_r] % LINE + W[case_r]
    for al in range(LINE):
        sums = set(s[(off[case_r] % LINE == al) & (W[case_r] <= TILE_CAP)].tolist())
        assert {v for v in (SLOTS - 2, SLOTS - 1, SLOTS) if v - al <= TILE_CAP} <= sums, al
    assert set(W_PIECES) <= set(W.tolist())
    # runs one window short of repeat_length, exactly long enough and one more, and a low window on either side of every run
    n_rep = np.diff(want["rep_offset"])
    assert set(n_rep[case_r].tolist()) == {0, 1} and np.all(n_rep[np.setdiff1d(np.arange(W.size), case_r)] == 0)
    assert set(np.unique(want["cov"]).tolist()) == {p.high_cov - 1, p.high_cov}
    # the case reads are what the generator says they are
    for (r, al, w, pl) in cases[:: max(1, len(cases) // 500)]:
        assert off[r] % LINE == al and W[r] == w and got.get((al, w_class(al, w), pl), 0) >= 1


def test_mixed_tiles_hold_what_they_say():
    p, cols = mixed_tiles()
    want = _oracle(p, cols)
    W = np.diff(want["cov_offset"])
    assert W.size == 20000
    for lo, hi in ((0, 0), (1, 1), (3, 3), (31, 31), (32, 32), (33, 33), (500, 700), (1500, 2100)):
        assert int(((W >= lo) & (W <= hi)).sum()) >= 100, (lo, hi)
    pair = W[:-1] + W[1:]
    near = (W[:-1] >= 1500) & (np.abs(pair - TILE_CAP) <= 40)
    assert int(near.sum()) >= 300
    # ... on both sides of every cut the two origins make: the pair fits behind 0 ... 31 slots or does not
    assert int((near & (pair <= SLOTS - 1 - 31)).sum()) >= 20 and int((near & (pair > SLOTS - 1 - 31) & (pair <= TILE_CAP)).sum()) >= 20
    assert int((near & (pair > TILE_CAP)).sum()) >= 20
    assert int(((W[:-1] == 0) & (W[1:] >= 1500)).sum()) >= 20     # a zero-length read in front of a long one
    assert np.diff(want["rep_offset"]).max() >= 1 and want["cov"].max() >= p.high_cov
    for n_runs in (2, 4):
        c2 = in_runs(cols, n_runs)
        starts = np.flatnonzero(np.diff(c2[1]) < 0)
        assert starts.size == n_runs - 1
        w2 = _oracle(p, c2)
        assert np.array_equal(w2["cov"], want["cov"]) and np.array_equal(w2["rep_s"], want["rep_s"])


def test_deep_tile_begins_off_a_line():
    p, cols = deep_tile()
    want = _oracle(p, cols)
    assert want["cov_offset"][2] % LINE != 0 and want["cov"].max() >= 32768
    assert M >= 2
