"""GPU: raft_hip_low_coverage (raft_amd/csrc/low_cov.hpp) -- the runs of consecutive windows with coverage <= low_cov of every read of a
finished pass, as CSR by read with per-read counts, class flags and totals -- exact against the definition restated on the oracle's
cov[] (tests/test_low_cov_cases.py want_low): at every unit boundary of the kernels, in every output width, at the encodings' limits,
on the golden fixtures, around the uncovered mark, under every run_cap, and in every state of the context."""
import ctypes as C
import json
import os

import numpy as np
import pytest
from raft_testlib import GOLDEN, assert_same_result, oracle_run
from test_gpu_read_stats import stacked
from test_low_cov_cases import HEAD, RESO, RUN_CAP_DELTAS, TAIL, UNCOVERED, cover, low_cases, same_low, want_low
from test_read_stats_cases import overlaps_for

from raft_amd.params import RaftParams

pytestmark = pytest.mark.gpu
WIDTHS = (4, 1, 2, 8)          # int32, byte codes, uint16 codes, four-bit steps (RAFT_HIP_COV_DELTA4)
MAN = json.load(open(os.path.join(GOLDEN, "manifest.json")))


def check_all_widths(p, cols, what, low_covs, want=None, widths=WIDTHS, permille=800):
    """One context, one pass per width over the same inputs, low_coverage under every low_cov; returns {width: summary}."""
    from raft_amd import engine
    if want is None:
        want = oracle_run(p, *cols)
    exp = {c: want_low(want, cols[0], p.reso, c, permille) for c in low_covs}
    out = {}
    eng = engine.Engine(p, device=0)
    try:
        for w in widths:
            eng.set_output_width(w)
            eng.run_host(*cols)
            out[w] = eng.finish()
            for c in low_covs:
                same_low(eng.low_coverage(c, permille), exp[c], f"{what}, width {w}, low_cov {c}")
            assert eng.last_low_coverage_seconds >= 0.0
    finally:
        eng.close()
    return out


# ---- run shapes -------------------------------------------------------------------------------------------------------------------------

CASES = low_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_run_shapes(name):
    windows, depth = CASES[name]
    cols = cover(windows, depth)
    p = RaftParams(est_cov=30, symmetric_mode=1)
    want = oracle_run(p, *cols)
    assert np.array_equal(want["cov"], depth)
    res = check_all_widths(p, cols, name, (0, 1, 2), want=want)
    assert res[4].n_bins == sum(windows) and res[4].n_reads == len(windows)


def test_no_reads():
    from raft_amd import engine
    e = [np.empty(0, np.int32)] * 7
    eng = engine.Engine(RaftParams(est_cov=3), device=0)
    for w in WIDTHS:
        eng.set_output_width(w)
        eng.run_host(*e)
        s = eng.finish()
        got = eng.low_coverage()
        assert s.n_reads == 0 and got["n_runs"] == 0 and list(got["low_offset"]) == [0], w
        assert all(got[k].size == 0 for k in ("low_s", "low_e", "low_windows", "low_flags")), w
    eng.close()


def _raw(eng, low_cov, permille, run_cap, n_reads, with_runs=True):
    """raft_hip_low_coverage as the ABI has it: the code, the summary and the arrays (filled with -1 before the call)."""
    from raft_amd import engine
    sm = engine._LowSummary()
    cap = max(run_cap, 0)
    off = np.full(n_reads + 1, -1, np.int64)
    s, e = np.full(cap + 1, -1, np.int32), np.full(cap + 1, -1, np.int32)
    win, fl = np.full(n_reads, -1, np.int32), np.full(n_reads, 255, np.uint8)
    P = lambda a: C.c_void_p(a.ctypes.data)
    rc = engine.load_side_library("low").raft_hip_low_coverage(eng._ctx, low_cov, permille, run_cap, P(off), P(s) if with_runs else None, P(e) if with_runs else None,
                                        P(win), P(fl), C.byref(sm), None)
    return rc, sm, off, s, e, win, fl


def test_run_cap_below_at_and_above_the_run_total():
    from raft_amd import engine
    windows, depth = CASES["head_interior_tail"]
    cols = cover(windows, depth)
    p = RaftParams(est_cov=30, symmetric_mode=1)
    exp = want_low(oracle_run(p, *cols), cols[0], RESO, 0, 800)
    n = exp["n_runs"]
    assert n >= 2
    eng = engine.Engine(p, device=0)
    eng.run_host(*cols); eng.finish()
    rc, sm, off, s, e, win, fl = _raw(eng, 0, 800, 0, len(windows), with_runs=False)          # the size query always succeeds
    assert rc == 0 and sm.n_runs == n
    for delta in RUN_CAP_DELTAS:
        rc, sm, off, s, e, win, fl = _raw(eng, 0, 800, n + delta, len(windows))
        assert sm.n_runs == n and sm.low_windows == exp["total_low_windows"] and sm.reads_interior == exp["reads_interior"]
        assert np.array_equal(off, exp["low_offset"]) and np.array_equal(win, exp["low_windows"]) and np.array_equal(fl, exp["low_flags"])
        if delta < 0:
            assert rc == engine.ERR_TOO_LARGE and (s == -1).all() and (e == -1).all()            # nothing of the two is copied
        else:
            assert rc == 0 and np.array_equal(s[:n], exp["low_s"]) and np.array_equal(e[:n], exp["low_e"])
            assert (s[n:] == -1).all() and (e[n:] == -1).all()
    eng.close()


# ---- the code limits --------------------------------------------------------------------------------------------------------------------

def test_low_cov_on_both_sides_of_the_code_limits():
    """Coverage 254, 255, 256, 65,534, 65,535 and 65,536 on known reads; low_cov below each code's limit reads the codes in place, at or
    above it the int32 route answers: the same either way."""
    from raft_amd import engine
    counts = [254, 255, 256, 65534, 65535, 65536]
    cols = stacked(counts)
    p = RaftParams(est_cov=30, symmetric_mode=1)
    want = oracle_run(p, *cols)
    for i, c in enumerate(counts):
        assert (want["cov"][want["cov_offset"][i]:want["cov_offset"][i + 1]] == c).all()
    low_covs = (0, 2, 253, 254, 255, 256, 65533, 65534, 65535, 65536, 2 ** 31 - 1)
    res = check_all_widths(p, cols, "code limits", low_covs, want=want)
    assert all(s.flags & engine.SUM_DEEP_TILES for s in res.values())
    for c, n_low in ((253, 1), (254, 2), (255, 3), (256, 4), (65534, 5), (65535, 6), (65536, 7)):
        assert want_low(want, cols[0], p.reso, c, 800)["n_runs"] == n_low          # (the plain read behind them has coverage 2)


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["s300_default", "s60_ultralong", "edge_reads", "s150_reso1"])
def test_golden_fixtures(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    p = RaftParams(**MAN["synthetic"][name]["params"])
    cols = [z[k] for k in ("read_len", "qid", "qs", "qe", "tid", "ts", "te")]
    want = oracle_run(p, *cols)
    high_cov = want["high_cov"]
    assert high_cov >= 1
    W = np.diff(want["cov_offset"])
    from raft_amd import engine
    eng = engine.Engine(p, device=0)
    try:
        for w in WIDTHS:
            eng.set_output_width(w)
            eng.run_host(*cols)
            eng.finish()
            hist = eng.coverage_histogram()
            for c in (0, high_cov - 1):
                got = eng.low_coverage(c)
                same_low(got, want_low(want, cols[0], p.reso, c, 800), f"{name}, width {w}, low_cov {c}")
                assert int(got["low_windows"].sum()) == int(hist[:c + 1].sum()), (name, w, c)
            # every window is either below high_cov or at or above it
            assert np.array_equal(got["low_windows"].astype(np.int64) + eng.read_stats(high_cov)["high_windows"], W), (name, w)
    finally:
        eng.close()


# ---- the uncovered mark -----------------------------------------------------------------------------------------------------------------

def test_uncovered_at_one_below_and_one_above_the_mark():
    """reso 1, reads of 1000 bases whose first k bases nobody covers: 1000 * k > permille * 1000 exactly when k > permille."""
    from raft_amd import engine
    ks = [0, 1, 799, 800, 801, 999, 1000]
    L = 1000
    depth = np.concatenate([(np.arange(L) >= k).astype(np.int64) for k in ks])
    cols = cover([L] * len(ks), depth, reso=1, short=0)
    p = RaftParams(est_cov=30, symmetric_mode=1, reso=1)
    want = oracle_run(p, *cols)
    assert np.array_equal(want["cov"], depth)
    eng = engine.Engine(p, device=0)
    try:
        for w in WIDTHS:
            eng.set_output_width(w)
            eng.run_host(*cols); eng.finish()
            for permille in (0, 800, 1000):
                got = eng.low_coverage(0, permille)
                same_low(got, want_low(want, cols[0], 1, 0, permille), f"width {w}, permille {permille}")
                assert list((got["low_flags"] & UNCOVERED) != 0) == [k > permille for k in ks], (w, permille)
                assert got["reads_uncovered"] == sum(k > permille for k in ks)
            assert list(got["low_flags"] & (HEAD | TAIL)) == [0] + [HEAD] * 5 + [HEAD | TAIL]
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
        eng.low_coverage()
    assert e.value.code == engine.ERR_STATE
    eng.run_host(*cols)
    eng.finish()
    want = oracle_run(p, *cols)
    same_low(eng.low_coverage(), want_low(want, cols[0], p.reso, 0, 800), "after finish")
    for args in ((-1, 800), (0, -1), (0, 1001)):
        with pytest.raises(engine.RaftError) as e:
            eng.low_coverage(*args)
        assert e.value.code == engine.ERR_PARAM
    eng.run_pipelined(*cols[:4], n_chunks=3)                        # host to host: the context holds no pass afterwards
    with pytest.raises(engine.RaftError) as e:
        eng.low_coverage()
    assert e.value.code == engine.ERR_STATE
    bad = [c.copy() for c in cols]
    bad[3][0] = bad[0][bad[1][0]] + 500                             # a record reaching past its read: a data error
    eng.run_host(*bad)
    with pytest.raises(engine.RaftError) as e:
        eng.finish()
    assert e.value.code == engine.ERR_COORD
    with pytest.raises(engine.RaftError) as e:
        eng.low_coverage()
    assert e.value.code == engine.ERR_STATE
    eng.run_host(*cols)
    eng.finish()
    same_low(eng.low_coverage(1, 0), want_low(want, cols[0], p.reso, 1, 0), "after the error")
    eng.close()


@pytest.mark.parametrize("width", WIDTHS)
def test_the_pass_is_left_as_it_is(width):
    from raft_amd import engine
    p = RaftParams(est_cov=3)
    cols = overlaps_for([700, 33, 1500, 2, 4093, 64] * 9, 1, per_read=6)
    want = oracle_run(p, *cols)
    exp = want_low(want, cols[0], p.reso, 1, 800)
    assert exp["n_runs"] > 0
    eng = engine.Engine(p, device=0)
    eng.set_output_width(width)
    eng.run_host(*cols); s = eng.finish()
    a, b = eng.low_coverage(1), eng.low_coverage(1)
    same_low(a, exp, f"width {width}")
    same_low(b, a, f"the second call, width {width}")                # (the device arrays are cleared at every call)
    assert_same_result(_full(eng, s), want, f"fetch after low_coverage, width {width}")
    same_low(eng.low_coverage(1), exp, f"after the fetch, width {width}")
    same_low(eng.low_coverage(70000), want_low(want, cols[0], p.reso, 70000, 800), f"above both code limits, width {width}")
    assert_same_result(_full(eng, s), want, f"fetch after the int32 route, width {width}")
    eng.close()


def test_low_coverage_hands_out_no_geometry():
    """A low_coverage call between two identical run_device passes leaves the second one speculated on kept geometry."""
    import torch
    from raft_amd import engine
    from test_gpu_speculate import _set
    p = RaftParams(est_cov=8, symmetric_mode=1)
    rl, (qid, a, b) = _set(31)
    want = oracle_run(p, rl, qid, a, b, qid, a, b); want["symmetric"] = 1      # (asserted by the parameters, not detected)
    exp = want_low(want, rl, p.reso, 0, 800)
    dev = [torch.from_numpy(x).to("cuda:0") for x in (rl, qid, a, b)]
    eng = engine.Engine(p, device=0)
    for it in range(2):
        eng.run_device(*dev); s = eng.finish()
        same_low(eng.low_coverage(), exp, f"pass {it}")
    eng.run_device(*dev); s = eng.finish()
    assert s.flags & engine.SUM_SPECULATED and s.flags & engine.SUM_KEPT_GEOMETRY, s.flags
    same_low(eng.low_coverage(), exp, "the speculated pass")
    assert_same_result(_full(eng, s), want, "the speculated pass")
    eng.close()
