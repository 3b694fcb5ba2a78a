"""GPU: raft_hip_read_stats (raft_amd/csrc/read_stats.hpp) -- per read, the sum and the maximum of the finished pass's window coverage and
the windows at or above a threshold, reduced on the device from the form the pass wrote -- exact against the oracle's cov[] cut by its
cov_offset, in every output width, at the kernel's structural sizes (tests/test_read_stats_cases.py), at the encodings' limits, on the
golden fixtures, and in every state of the context."""
import json
import os

import numpy as np
import pytest
from raft_testlib import GOLDEN, assert_same_result, oracle_run
from test_read_stats_cases import constants, overlaps_for, segment_cases

from raft_amd.params import RaftParams

pytestmark = pytest.mark.gpu
WIDTHS = (4, 1, 2, 8)          # int32, byte codes, uint16 codes, four-bit steps (RAFT_HIP_COV_DELTA4)
MAN = json.load(open(os.path.join(GOLDEN, "manifest.json")))


def want_stats(want, threshold):
    """sum, max and count(>= threshold) of the oracle's cov[] per read."""
    cov = np.asarray(want["cov"], np.int64)
    off = np.asarray(want["cov_offset"], np.int64)
    cs = np.concatenate([[0], np.cumsum(cov)])
    ch = np.concatenate([[0], np.cumsum(cov >= threshold)])
    mx = np.zeros(off.size - 1, np.int64)
    some = off[1:] > off[:-1]
    if some.any():
        mx[some] = np.maximum.reduceat(cov, off[:-1][some])
    return {"cov_sum": cs[off[1:]] - cs[off[:-1]], "cov_max": mx, "high_windows": ch[off[1:]] - ch[off[:-1]]}


def check_stats(got, want, threshold, what):
    exp = want_stats(want, threshold)
    assert got["cov_sum"].dtype == np.int64 and got["cov_max"].dtype == np.int32 and got["high_windows"].dtype == np.int32
    for k in ("cov_sum", "cov_max", "high_windows"):
        assert got[k].shape == exp[k].shape, (what, k)
        bad = np.flatnonzero(got[k].astype(np.int64) != exp[k])
        assert bad.size == 0, f"{what}, threshold {threshold}: {k} differs on {bad.size} reads, first read {bad[0]}: got {got[k][bad[0]]} want {exp[k][bad[0]]}"


def check_all_widths(p, cols, what, thresholds=None, widths=WIDTHS, want=None):
    """One context, one pass per width over the same inputs, read_stats under every threshold; returns {width: summary}."""
    from raft_amd import engine
    if want is None:
        want = oracle_run(p, *cols)
    if thresholds is None:
        thresholds = (want["high_cov"], 1)
    out = {}
    eng = engine.Engine(p, device=0)
    try:
        for w in widths:
            eng.set_output_width(w)
            eng.run_host(*cols)
            s = eng.finish()
            for t in thresholds:
                got = eng.read_stats(t)
                check_stats(got, want, t, f"{what}, width {w}")
                assert int(got["cov_sum"].sum()) == s.total_coverage, (what, w)
                assert int(got["cov_max"].max(initial=0)) == int(np.max(want["cov"], initial=0)), (what, w)
            assert eng.last_read_stats_seconds >= 0.0
            out[w] = s
    finally:
        eng.close()
    return out


# ---- segment shapes ---------------------------------------------------------------------------------------------------------------------

CASES = segment_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_segment_shapes(name):
    windows = CASES[name]
    cols = overlaps_for(windows, 100 + len(name))
    res = check_all_widths(RaftParams(est_cov=1), cols, name, thresholds=(1, 2))
    assert res[4].n_bins == sum(windows) and res[4].n_reads == len(windows)
    if name == "grid_stride":
        k = constants()
        for w, S in k["span"].items():
            assert sum(windows) > S * k["kReadStatsMaxBlocks"], (w, "the capped grid covers the set in one step")


def test_no_reads():
    from raft_amd import engine
    e = [np.empty(0, np.int32)] * 7
    eng = engine.Engine(RaftParams(est_cov=3), device=0)
    for w in WIDTHS:
        eng.set_output_width(w)
        eng.run_host(*e)
        s = eng.finish()
        got = eng.read_stats()
        assert s.n_reads == 0 and all(got[k].size == 0 for k in ("cov_sum", "cov_max", "high_windows")), w
    eng.close()


# ---- values and thresholds --------------------------------------------------------------------------------------------------------------

def stacked(counts, windows=50, reso=50):
    """Read i with counts[i] identical full-length records: every window of it at counts[i] (and one plain read behind them)."""
    counts = list(counts) + [2]
    rl = np.full(len(counts), windows * reso, np.int32)
    qid = np.repeat(np.arange(len(counts)), counts).astype(np.int32)
    a = np.zeros(qid.size, np.int32)
    b = np.full(qid.size, windows * reso, np.int32)
    return [rl, qid, a, b, qid.copy(), a.copy(), b.copy()]


LIMIT_THRESHOLDS = (1, 2, 254, 255, 256, 257, 65534, 65535, 65536, 65537, 2 ** 31 - 1)


def test_values_and_thresholds_around_the_code_limits():
    """Coverage 254, 255, 256, 65,534, 65,535 and 65,536 on known windows; thresholds on both sides of each code's limit
    (threshold <= limit: the main kernel counts the window; limit < threshold <= value: the exception kernel does; threshold > value:
    nobody), 1 and 2^31 - 1."""
    from raft_amd import engine
    counts = [254, 255, 256, 65534, 65535, 65536]
    cols = stacked(counts)
    p = RaftParams(est_cov=30, symmetric_mode=1)
    want = oracle_run(p, *cols)
    for i, c in enumerate(counts):
        assert (want["cov"][want["cov_offset"][i]:want["cov_offset"][i + 1]] == c).all()
    res = check_all_widths(p, cols, "code limits", thresholds=LIMIT_THRESHOLDS, want=want)
    assert all(s.flags & engine.SUM_DEEP_TILES for s in res.values())


def test_a_byte_pass_most_of_whose_windows_are_listed():
    n, L, k = 300, 20000, 300
    rl = np.full(n, L, np.int32)
    rl[::7] = 2500                                        # (reads of 50 windows among those of 400: boundaries inside spans)
    qid = np.repeat(np.arange(n), k).astype(np.int32)
    a = np.zeros(qid.size, np.int32)
    b = rl[qid].copy()
    cols = [rl, qid, a, b, qid.copy(), a.copy(), b.copy()]
    p = RaftParams(est_cov=30, symmetric_mode=1)
    want = oracle_run(p, *cols)
    assert (want["cov"] >= 255).mean() > 0.9
    check_all_widths(p, cols, "k = 300 everywhere", thresholds=(1, 255, 256, 300, 301), want=want)


def test_a_pile_of_40000_on_one_read():
    from raft_amd import engine
    res = check_all_widths(RaftParams(est_cov=30, symmetric_mode=1), stacked([40000, 3]), "40000 deep", thresholds=(1, 4, 40000, 40001))
    assert all(s.flags & engine.SUM_DEEP_TILES for s in res.values())


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["s300_default", "s60_ultralong", "edge_reads", "s150_reso1"])
def test_golden_fixtures(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    p = RaftParams(**MAN["synthetic"][name]["params"])
    cols = [z[k] for k in ("read_len", "qid", "qs", "qe", "tid", "ts", "te")]
    want = oracle_run(p, *cols)
    from raft_amd import engine
    eng = engine.Engine(p, device=0)
    try:
        for w in WIDTHS:
            eng.set_output_width(w)
            eng.run_host(*cols)
            s = eng.finish()
            got = eng.read_stats()                        # threshold = high_cov
            check_stats(got, want, want["high_cov"], f"{name}, width {w}")
            assert s.high_cov == want["high_cov"]
            assert int(got["cov_sum"].sum()) == s.total_coverage
            assert int(got["cov_max"].max(initial=0)) == int(np.max(want["cov"], initial=0))
            # a repeat is a run of windows at or above high_cov that spans repeat_length
            has_repeat = np.diff(want["rep_offset"]) > 0
            assert (got["high_windows"][has_repeat].astype(np.int64) * p.reso >= p.repeat_length).all(), (name, w)
            check_stats(eng.read_stats(1), want, 1, f"{name}, width {w}")
    finally:
        eng.close()


# ---- state ------------------------------------------------------------------------------------------------------------------------------

def _full(eng, s):
    got = eng.fetch()
    got.update(symmetric=s.symmetric, high_cov=s.high_cov, total_coverage=s.total_coverage, total_windows=s.total_windows,
               total_repeat_length=s.total_repeat_length, total_read_length=s.total_read_length)
    return got


def test_call_order_and_parameters():
    from raft_amd import engine
    p = RaftParams(est_cov=3, symmetric_mode=1)
    cols = overlaps_for([500, 77, 1200] * 5, 3)
    eng = engine.Engine(p, device=0)
    with pytest.raises(engine.RaftError) as e:                      # no pass at all
        eng.read_stats()
    assert e.value.code == engine.ERR_STATE
    eng.run_host(*cols)
    eng.finish()
    want = oracle_run(p, *cols)
    check_stats(eng.read_stats(), want, want["high_cov"], "after finish")
    for t in (0, -1):
        with pytest.raises(engine.RaftError) as e:
            eng.read_stats(t)
        assert e.value.code == engine.ERR_PARAM
    eng.run_pipelined(*cols[:4], n_chunks=3)                        # host to host: the context holds no pass afterwards
    with pytest.raises(engine.RaftError) as e:
        eng.read_stats()
    assert e.value.code == engine.ERR_STATE
    bad = [c.copy() for c in cols]
    bad[3][0] = bad[0][bad[1][0]] + 500                             # a record reaching past its read: a data error
    eng.run_host(*bad)
    with pytest.raises(engine.RaftError) as e:
        eng.finish()
    assert e.value.code == engine.ERR_COORD
    with pytest.raises(engine.RaftError) as e:
        eng.read_stats()
    assert e.value.code == engine.ERR_STATE
    eng.run_host(*cols)
    eng.finish()
    check_stats(eng.read_stats(2), want, 2, "after the error")
    eng.close()


@pytest.mark.parametrize("width", WIDTHS)
def test_the_pass_is_left_as_it_is(width):
    from raft_amd import engine
    p = RaftParams(est_cov=3)
    cols = overlaps_for([700, 33, 1500, 2, 4093, 64] * 9, 1, per_read=6)
    want = oracle_run(p, *cols)
    eng = engine.Engine(p, device=0)
    eng.set_output_width(width)
    eng.run_host(*cols); s = eng.finish()
    a, b = eng.read_stats(3), eng.read_stats(3)
    check_stats(a, want, 3, f"width {width}")
    assert all(np.array_equal(a[k], b[k]) for k in a)               # (the device arrays are cleared at every call)
    assert_same_result(_full(eng, s), want, f"fetch after read_stats, width {width}")
    check_stats(eng.read_stats(3), want, 3, f"after the fetch, width {width}")
    eng.close()


def test_read_stats_hands_out_no_geometry():
    """A read_stats call between two identical run_device passes leaves the second one speculated on kept geometry."""
    import torch
    from raft_amd import engine
    from test_gpu_speculate import _set
    p = RaftParams(est_cov=8, symmetric_mode=1)
    rl, (qid, a, b) = _set(31)
    want = oracle_run(p, rl, qid, a, b, qid, a, b); want["symmetric"] = 1      # (asserted by the parameters, not detected)
    dev = [torch.from_numpy(x).to("cuda:0") for x in (rl, qid, a, b)]
    eng = engine.Engine(p, device=0)
    for it in range(2):
        eng.run_device(*dev); s = eng.finish()
        check_stats(eng.read_stats(), want, want["high_cov"], f"pass {it}")
    eng.run_device(*dev); s = eng.finish()
    assert s.flags & engine.SUM_SPECULATED and s.flags & engine.SUM_KEPT_GEOMETRY, s.flags
    check_stats(eng.read_stats(), want, want["high_cov"], "the speculated pass")
    assert_same_result(_full(eng, s), want, "the speculated pass")
    eng.close()
