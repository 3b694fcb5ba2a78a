"""Input sets for the question where a wave tile's int32 array begins in cov[] (raft_amd/csrc/pileup_wave.hpp `a0`): on a 4-window
boundary, as it does, or on a 128-byte line (32 windows) when the tile still fits behind the line's slots.

Nothing here runs on a GPU.  tests/test_line_cases.py pins what the sets hold (from the oracle's side), tests/test_gpu_line_aligned.py
runs them through every input form.  All sets use reso 1 (a window is a base), self overlaps sorted by read id (only the query side
piles up) and small parameters; what must come out is the oracle's.
"""
import numpy as np
from raft_testlib import TILE_CAP

from raft_amd.params import RaftParams

SLOTS = TILE_CAP + 4          # pileup_wave.hpp: slots of a wave's LDS array; a tile's last window sits at slot SLOTS - 2 at the most
LINE = 32                     # windows of a 128-byte line of int32 coverage
M = 6                         # repeat_length in windows
W_TILE = (2047,) + tuple(range(4060, TILE_CAP + 1))       # one read, one tile: two reads of 2047 windows do not fit one array
W_PIECES = (TILE_CAP + 1, TILE_CAP + 2, 2 * TILE_CAP, 2 * TILE_CAP + 1, 3 * TILE_CAP)
PLACEMENTS = ("first", "last", "line")


def line_params(H=2):
    return RaftParams(reso=1, est_cov=H, cov_mul=1.0, repeat_length=M, interval_length=500, read_length=1000, overlap_length=0,
                      flanking_length=3, symmetric_mode=1)


def w_class(al, W):
    """How a read of W windows that begins a tile at offset mod 32 = al meets the array."""
    if W > TILE_CAP:
        return f"pieces {W}"
    if W == 2047:
        return "2047"
    s = al + W
    return "room" if s <= SLOTS - 2 else "last fit" if s == SLOTS - 1 else "first fallback" if s == SLOTS else "beyond"


def feasible_classes(al):
    out = ["2047", "room"] + [f"pieces {W}" for W in W_PIECES]
    if al + TILE_CAP >= SLOTS - 1:
        out.append("last fit")
    if al + TILE_CAP >= SLOTS:
        out.append("first fallback")
    if al + TILE_CAP > SLOTS:
        out.append("beyond")
    return out


def run_of(placement, al, W, L):
    """The read's one run of high windows [s, e): windows 0 ... L - 1, ending on the last window, or across windows 31 - al | 32 - al
    (the first line boundary of the array's first row when the array begins on a line)."""
    if placement == "first":
        return 0, L
    if placement == "last":
        return W - L, W
    s = LINE - al - min(3, LINE - al)
    return s, s + L


def single_read_tiles():
    """-> (params, [read_len, qid, qs, qe], per case read: index, residue, W, placement).  Every residue of cov_offset mod 32, reached
    by a pad read in front (2047 windows and up: it has a tile of its own as well), crossed with every W of W_TILE + W_PIECES and the
    three placements of the run; one record over the whole read (every window at high_cov - 1: a low window on either side of the
    run) and one over the run, M - 1, M or M + 1 windows long."""
    rl, qid, qs, qe, cases = [], [], [], [], []
    off = 0

    def add(W, runs):
        nonlocal off
        r = len(rl)
        rl.append(W)
        for (s, e) in [(0, W)] + runs:
            qid.append(r); qs.append(s); qe.append(e)
        off += W
        return r

    i = 0
    for al in range(LINE):
        for W in W_TILE + W_PIECES:
            for pl in PLACEMENTS:
                pad = 2047 + (al - (off + 2047)) % LINE
                add(pad, [])
                assert off % LINE == al
                L = M - 1 + i % 3
                i += 1
                cases.append((add(W, [run_of(pl, al, W, L)]), al, W, pl))
    cols = [np.array(x, np.int32) for x in (rl, qid, qs, qe)]
    return line_params(), cols, cases


def mixed_tiles(n_reads=20000, seed=77):
    """Tiles of several reads: a seeded mix of reads of 0, 1, 3, 31 ... 33, 500 ... 700 and 1500 ... 2100 windows -- zero-length reads
    wherever a tile may begin, and every eighth long read followed by a partner that brings the pair to within 40 windows of TILE_CAP
    on either side, so that a cut that leaves room for a line's slots drops the partner where the 4-window cut kept it.  Three random
    records per read; high_cov = 2."""
    rng = np.random.default_rng(seed)
    W = np.empty(n_reads, np.int64)
    kind = rng.choice(6, n_reads, p=[0.08, 0.08, 0.08, 0.16, 0.32, 0.28])
    W[kind == 0] = 0
    W[kind == 1] = 1
    W[kind == 2] = 3
    W[kind == 3] = rng.integers(31, 34, int((kind == 3).sum()))
    W[kind == 4] = rng.integers(500, 701, int((kind == 4).sum()))
    W[kind == 5] = rng.integers(1500, 2101, int((kind == 5).sum()))
    long_ = np.flatnonzero(kind == 5)[::8]
    long_ = long_[long_ + 1 < n_reads]
    W[long_ + 1] = TILE_CAP - W[long_] + rng.integers(-40, 41, long_.size)
    n = np.where(W > 0, 3, 0)
    qid = np.repeat(np.arange(n_reads), n)
    Wr = W[qid]
    qs = (rng.random(qid.size) * Wr).astype(np.int64)
    qe = qs + 1 + (rng.random(qid.size) * (Wr - qs)).astype(np.int64)
    qe = np.minimum(qe, Wr)
    assert np.all((qs < qe) & (qe <= Wr))
    return line_params(), [W.astype(np.int32), qid.astype(np.int32), qs.astype(np.int32), qe.astype(np.int32)]


def deep_tile(m=40000, seed=9):
    """40,000 intervals on one read (tests/test_gpu_deep.py) whose first window is not on a line."""
    rng = np.random.default_rng(seed)
    rl = np.array([30000, 12350, 50000, 8000], np.int32)
    qid = np.concatenate([np.zeros(50, np.int32), np.full(m, 2, np.int32), np.full(30, 3, np.int32)])
    qs = np.zeros(qid.size, np.int32); qe = np.zeros(qid.size, np.int32)
    qs[50:50 + m] = rng.integers(0, 20000, m)
    qe[50:50 + m] = qs[50:50 + m] + rng.integers(20000, 30000, m)
    qs[:50] = rng.integers(0, 10000, 50); qe[:50] = qs[:50] + 5000
    qs[50 + m:] = 100; qe[50 + m:] = 7000
    return RaftParams(est_cov=30, symmetric_mode=1), [rl, qid, qs, qe]


def in_runs(cols, n_runs, seed=5):
    """The same records as n_runs runs sorted by read id, one after the other (what a handful of sorted files give)."""
    rl, qid, qs, qe = cols
    if n_runs == 1:
        return [rl, qid, qs, qe]
    run = np.random.default_rng(seed).integers(0, n_runs, qid.size)
    run[:n_runs] = np.arange(n_runs)[:run.size]                  # (every run exists)
    order = np.lexsort((qid, run))
    return [rl, qid[order], qs[order], qe[order]]


def census(cov_offset, cov, high_cov):
    """From the oracle's arrays alone: {(residue, W class, placement): reads}, over the reads that hold a run of high windows."""
    off = np.asarray(cov_offset, np.int64)
    high = np.asarray(cov) >= high_cov
    out = {}
    for r in range(off.size - 1):
        o, W = int(off[r]), int(off[r + 1] - off[r])
        h = high[o:o + W]
        if W < 2047 or not h.any():
            continue
        al = o % LINE
        pl = [p for p, hit in (("first", h[0]), ("last", h[-1]), ("line", h[LINE - al - 1] and h[LINE - al])) if hit]
        for p in pl:
            key = (al, w_class(al, W), p)
            out[key] = out.get(key, 0) + 1
    return out
