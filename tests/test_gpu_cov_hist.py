"""GPU: raft_hip_cov_histogram (raft_amd/csrc/cov_hist.hpp) -- the histogram of a finished pass's window coverage, computed on the
device from the form the pass wrote -- bit-exact against  np.bincount(np.minimum(cov, 4095), minlength=4096)  on the oracle's cov[],
in every output width, at the kernel's structural sizes, under contention, at the encodings' limits and on realistic sets; and the
estimate read from it (raft_hip_estimate_coverage, Engine.estimate_from)."""
import os
import re

import numpy as np
import pytest
from raft_testlib import ROOT, assert_same_result, oracle_run
from test_cov_estimate import restate

from raft_amd.params import RaftParams

pytestmark = pytest.mark.gpu
BINS = 4096
WIDTHS = (4, 1, 2, 8)          # int32, byte codes, uint16 codes, four-bit steps (RAFT_HIP_COV_DELTA4)


def want_hist(cov):
    return np.bincount(np.minimum(np.asarray(cov, np.int64), BINS - 1), minlength=BINS).astype(np.int64)


def launch_constants():
    """The launch arithmetic of cov_hist.hpp, read from the header: threads per workgroup, the cap on workgroups, groups of loads a
    lane has in flight, and the windows of one group per element type (two 16-byte loads of int32, one of codes)."""
    text = open(os.path.join(ROOT, "raft_amd", "csrc", "cov_hist.hpp")).read()
    k = {name: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1)) for name in ("kCovHistThreads", "kCovHistMaxBlocks", "kCovHistInFlight")}
    vecs = {t: int(v) for t, v in re.findall(r"struct CovHistIn<(\w+)> \{ static constexpr int vecs = (\d+);", text)}
    lane_windows = {4: vecs["int32_t"] * 16 // 4, 2: vecs["uint16_t"] * 16 // 2, 1: vecs["uint8_t"] * 16}
    return k["kCovHistThreads"], k["kCovHistMaxBlocks"], k["kCovHistInFlight"], lane_windows


def self_overlaps(windows, seed, per_read=3, reso=50):
    """Reads of the given window counts with a few random self overlaps each (tid = qid: only the query side piles up)."""
    rng = np.random.default_rng(seed)
    W = np.asarray(windows, np.int64)
    rl = (W * reso - rng.integers(0, reso, W.size)).astype(np.int32)
    qid = np.repeat(np.arange(W.size), per_read).astype(np.int32)
    a = (rng.random(qid.size) * rl[qid]).astype(np.int32)
    b = np.minimum(rl[qid], a + 1 + (rng.random(qid.size) * rl[qid]).astype(np.int32)).astype(np.int32)
    return [rl, qid, a, b, qid.copy(), a.copy(), b.copy()]


def check_all_widths(p, cols, what, widths=WIDTHS, want=None):
    """One context, one pass per width over the same inputs; returns {width: (hist, summary)}."""
    from raft_amd import engine
    if want is None:
        want = oracle_run(p, *cols)
    wh = want_hist(want["cov"])
    out = {}
    eng = engine.Engine(p, device=0)
    try:
        for w in widths:
            eng.set_output_width(w)
            eng.run_host(*cols)
            s = eng.finish()
            h = eng.coverage_histogram()
            assert h.dtype == np.int64 and h.shape == (BINS,)
            bad = np.flatnonzero(h != wh)
            assert bad.size == 0, f"{what}, width {w}: {bad.size} bins differ, first bin {bad[0]}: got {h[bad[0]]} want {wh[bad[0]]}"
            assert int(h.sum()) == s.n_bins == want["cov"].size, (what, w)
            if h[BINS - 1] == 0:
                assert int((np.arange(BINS, dtype=np.int64) * h).sum()) == s.total_coverage, (what, w)
            assert eng.last_histogram_seconds >= 0.0
            out[w] = (h, s)
    finally:
        eng.close()
    return out


# ---- structural sizes -------------------------------------------------------------------------------------------------------------------

STRUCT = {
    "one_window": [1], "five": [5], "six": [6], "seven": [7],                        # below a lane's 8 windows; n_bins = 1, 2, 3 mod 4
    "eleven": [3, 4, 4], "nine": [9], "seventeen": [17], "thirty_five": [16, 16, 3],  # around one group of int32 and of bytes
    "below_a_workgroup_step": [100, 131, 900, 1018],                                   # 2149 windows: fewer than 256 lanes x 16
    "three_workgroups": [4093] * 5 + [2],                                              # 20467 = 3 mod 4
    "many_workgroups": [1237] * 211 + [6],                                             # 261013 = 1 mod 4
}


@pytest.mark.parametrize("name", sorted(STRUCT))
def test_structural_sizes(name):
    cols = self_overlaps(STRUCT[name], 100 + len(name))
    check_all_widths(RaftParams(est_cov=3), cols, name)


def test_no_reads():
    from raft_amd import engine
    e = [np.empty(0, np.int32)] * 7
    eng = engine.Engine(RaftParams(est_cov=3), device=0)
    for w in WIDTHS:
        eng.set_output_width(w)
        eng.run_host(*e)
        s = eng.finish()
        h = eng.coverage_histogram()
        assert s.n_bins == 0 and h.shape == (BINS,) and not h.any(), w
    eng.close()


def test_grid_stride_loop_iterates():
    """More windows than the capped grid takes in one step of its main loop, in every element type: the loop body runs more than once."""
    threads, max_blocks, in_flight, lane_windows = launch_constants()
    windows = [4001] * 2100
    n_bins = sum(windows)
    for width, lw in lane_windows.items():
        # (groups of lw windows; the capped grid takes in_flight groups per lane and step)
        assert n_bins // lw > in_flight * max_blocks * threads, (width, "the capped grid covers the set in one step")
    res = check_all_widths(RaftParams(est_cov=3), self_overlaps(windows, 7, per_read=4), "grid stride")
    assert res[4][1].n_bins == n_bins


# ---- contention -------------------------------------------------------------------------------------------------------------------------

def flat_reads(k, alternate):
    n, L, reso = 2000, 20000, 50
    rl = np.full(n, L, np.int32)
    if not alternate:                       # k identical full-length records: every window at k
        qid = np.repeat(np.arange(n), k).astype(np.int32)
        a = np.zeros(qid.size, np.int32)
        b = np.full(qid.size, L, np.int32)
    else:                                   # k records on every other window: k, 0, k, 0 ... -- no two neighbours equal
        starts = np.arange(0, L, 2 * reso, dtype=np.int32)
        qid = np.repeat(np.arange(n), k * starts.size).astype(np.int32)
        a = np.tile(np.repeat(starts, k), n).astype(np.int32)
        b = a + reso
    return [rl, qid, a, b, qid.copy(), a.copy(), b.copy()]


@pytest.mark.parametrize("k,alternate", [(3, False), (300, False), (3, True)], ids=["k3", "k300", "k3_every_other_window"])
def test_contention(k, alternate):
    cols = flat_reads(k, alternate)
    res = check_all_widths(RaftParams(est_cov=30, symmetric_mode=1), cols, f"k={k} alternate={alternate}")
    h = res[4][0]
    n_win = 2000 * 400
    if alternate:
        assert h[k] == n_win // 2 and h[0] == n_win // 2
    else:
        assert h[min(k, BINS - 1)] == n_win


# ---- the encodings' limits --------------------------------------------------------------------------------------------------------------

def stacked(counts, windows=400, reso=50):
    """Read i with counts[i] identical full-length records (and one plain read behind them)."""
    counts = list(counts) + [2]
    rl = np.full(len(counts), windows * reso, np.int32)
    qid = np.repeat(np.arange(len(counts)), counts).astype(np.int32)
    a = np.zeros(qid.size, np.int32)
    b = np.full(qid.size, windows * reso, np.int32)
    return [rl, qid, a, b, qid.copy(), a.copy(), b.copy()]


def test_values_beyond_a_byte_and_beyond_the_last_bin():
    res = check_all_widths(RaftParams(est_cov=30, symmetric_mode=1), stacked([300, 5000, 255, 254, 4095, 4094]), "300 / 5000")
    for w, (h, s) in res.items():
        assert h[300] == 400 and h[255] == 400 and h[254] == 400 and h[4094] == 400, w
        assert h[BINS - 1] == 800, w           # 5000 and 4095: the clamp bin


def test_value_beyond_two_bytes_on_the_deep_kernel():
    from raft_amd import engine
    res = check_all_widths(RaftParams(est_cov=30, symmetric_mode=1), stacked([66000, 65535, 65534]), "66000")
    for w, (h, s) in res.items():
        assert s.flags & engine.SUM_DEEP_TILES, w
        assert h[BINS - 1] == 1200 and h[2] == 400, w


# ---- realistic sets ---------------------------------------------------------------------------------------------------------------------

_sets = {}


def realistic(C, S, mode):
    """make_overlaps(4000, coverage=C, seed=S) as the three kinds of pass; the oracle's result is computed once per set."""
    from raft_amd.synth import make_overlaps
    key = (C, S, mode)
    if key not in _sets:
        o = make_overlaps(4000, coverage=C, seed=S, **{"symmetric": {}, "non_symmetric": {"symmetric": False}, "shuffled": {"shuffle": True}}[mode])
        cols = [c.numpy() for c in (o.read_len,) + o.columns()]
        p = RaftParams(est_cov=C)
        _sets[key] = (p, cols, oracle_run(p, *cols))
    return _sets[key]


@pytest.mark.parametrize("mode", ["symmetric", "non_symmetric", "shuffled"])
@pytest.mark.parametrize("C,S", [(20, 1), (20, 2), (30, 3), (30, 4)])
def test_realistic_sets(C, S, mode):
    from raft_amd import engine
    p, cols, want = realistic(C, S, mode)
    res = check_all_widths(p, cols, f"{C}x seed {S} {mode}", want=want)
    assert res[4][1].interval_path == (0 if mode == "symmetric" else 1)      # (target sides, or no sorted runs: the general bucketing)
    assert res[4][1].symmetric == (0 if mode == "non_symmetric" else 1)
    for w, (h, s) in res.items():
        e = engine.estimate_coverage(h)
        r = restate(want_hist(want["cov"]))
        assert (e.est_cov, e.median, e.windows, e.windows_covered, e.windows_clamped) == \
            (r["est_cov"], r["median"], r["windows"], r["windows_covered"], r["windows_clamped"]), w
        assert abs(e.est_cov - C) <= 0.15 * C, (w, e)


# ---- state ------------------------------------------------------------------------------------------------------------------------------

def _full(eng, s):
    got = eng.fetch()
    got.update(symmetric=s.symmetric, high_cov=s.high_cov, total_coverage=s.total_coverage, total_windows=s.total_windows,
               total_repeat_length=s.total_repeat_length, total_read_length=s.total_read_length)
    return got


@pytest.mark.parametrize("width", WIDTHS)
def test_repeated_calls_other_data_and_fetch_afterwards(width):
    from raft_amd import engine
    p = RaftParams(est_cov=3)
    cols1 = self_overlaps([700, 33, 1500, 2, 4093, 64] * 9, 1, per_read=6)
    cols2 = self_overlaps([90, 4100, 5] * 11, 2, per_read=9)
    want1, want2 = oracle_run(p, *cols1), oracle_run(p, *cols2)
    eng = engine.Engine(p, device=0)
    eng.set_output_width(width)
    eng.run_host(*cols1); s = eng.finish()
    h1, h1b = eng.coverage_histogram(), eng.coverage_histogram()
    assert np.array_equal(h1, want_hist(want1["cov"])) and np.array_equal(h1b, h1)       # (the device array is cleared at every call)
    assert_same_result(_full(eng, s), want1, f"fetch after the histogram, width {width}")
    assert np.array_equal(eng.coverage_histogram(), h1)                                   # ... and after the fetch
    eng.run_host(*cols2); s = eng.finish()
    assert np.array_equal(eng.coverage_histogram(), want_hist(want2["cov"]))
    assert_same_result(_full(eng, s), want2, f"second set, width {width}")
    eng.close()


def test_call_order():
    from raft_amd import engine
    p = RaftParams(est_cov=3, symmetric_mode=1)
    cols = self_overlaps([500, 77, 1200] * 5, 3)
    eng = engine.Engine(p, device=0)
    with pytest.raises(engine.RaftError) as e:                      # no pass at all
        eng.coverage_histogram()
    assert e.value.code == engine.ERR_STATE
    eng.run_host(*cols)
    with pytest.raises(engine.RaftError) as e:                      # a pass in flight
        eng.coverage_histogram()
    assert e.value.code == engine.ERR_STATE
    eng.finish()
    want = want_hist(oracle_run(p, *cols)["cov"])
    assert np.array_equal(eng.coverage_histogram(), want)
    # host to host through the chunked pipeline (an explicit chunk count is honoured from tiny inputs on): the context holds no pass
    # afterwards -- the histogram is valid exactly where raft_hip_fetch is
    eng.run_pipelined(*cols[:4], n_chunks=3)
    with pytest.raises(engine.RaftError) as e:
        eng.coverage_histogram()
    assert e.value.code == engine.ERR_STATE
    with pytest.raises(engine.RaftError) as e:
        eng.fetch()
    assert e.value.code == engine.ERR_STATE
    bad = [c.copy() for c in cols]
    bad[3][0] = bad[0][bad[1][0]] + 500                             # a record reaching past its read: a data error
    eng.run_host(*bad)
    with pytest.raises(engine.RaftError) as e:
        eng.finish()
    assert e.value.code == engine.ERR_COORD
    with pytest.raises(engine.RaftError) as e:
        eng.coverage_histogram()
    assert e.value.code == engine.ERR_STATE
    eng.close()


def test_the_histogram_hands_out_no_geometry():
    """A speculated pass keeps the per-read geometry of the pass before it unless somebody was handed the arrays: the histogram is
    not such a call, raft_hip_outputs_device is."""
    import torch
    from raft_amd import engine
    from test_gpu_speculate import _set
    p = RaftParams(est_cov=8, symmetric_mode=1)
    rl, (qid, a, b) = _set(31)
    want = want_hist(oracle_run(p, rl, qid, a, b, qid, a, b)["cov"])
    dev = [torch.from_numpy(x).to("cuda:0") for x in (rl, qid, a, b)]
    eng = engine.Engine(p, device=0)
    for it in range(2):
        eng.run_device(*dev); s = eng.finish()
        assert np.array_equal(eng.coverage_histogram(), want), it
    eng.run_device(*dev); s = eng.finish()
    assert s.flags & engine.SUM_SPECULATED and s.flags & engine.SUM_KEPT_GEOMETRY, s.flags
    assert np.array_equal(eng.coverage_histogram(), want)
    eng.outputs_device()
    eng.run_device(*dev); s = eng.finish()
    assert s.flags & engine.SUM_SPECULATED and not s.flags & engine.SUM_KEPT_GEOMETRY, s.flags
    assert np.array_equal(eng.coverage_histogram(), want)
    eng.close()


def test_estimate_from_sets_the_parameter():
    import dataclasses
    import torch
    from raft_amd import engine
    p0, cols, want0 = realistic(30, 3, "symmetric")
    p = dataclasses.replace(p0, est_cov=1)                          # a placeholder: create rejects 0
    dev = [torch.from_numpy(c).to("cuda:0") for c in cols]
    eng = engine.Engine(p, device=0)
    est = eng.estimate_from(*dev)
    r = restate(want_hist(want0["cov"]))
    assert est.est_cov == r["est_cov"] and est.est_cov > 0 and eng.params.est_cov == est.est_cov
    assert eng.last_histogram_seconds > 0.0
    eng.run_device(*dev); s = eng.finish()
    want = oracle_run(dataclasses.replace(p0, est_cov=est.est_cov), *cols)
    assert s.high_cov == want["high_cov"]
    assert_same_result(_full(eng, s), want, "the pass after estimate_from")
    eng.close()
