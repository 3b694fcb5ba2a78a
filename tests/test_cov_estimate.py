"""CPU: raft_hip_estimate_coverage (host arithmetic, no device) against its specification restated in numpy / Python integers,
and the binding's surface for the coverage histogram."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from raft_amd import engine


def restate(hist):
    """include/raft_hip.h, in Python integers: the smoothed mode of the covered, unclamped bins; the lower weighted median of the
    covered windows; the sums; the mean with the clamp bin counted at n - 1."""
    h = [int(x) for x in hist]
    n = len(h)
    c = [0] + h[1:n - 1] + [0]
    best, est = 0, 0
    for v in range(1, n - 1):
        s = c[v - 1] + c[v] + c[v + 1]
        if s > best:
            best, est = s, v
    covered = sum(h[1:])
    median, run = 0, 0
    if covered > 0:
        for v in range(1, n):
            run += h[v]
            if 2 * run >= covered:
                median = v
                break
    total = sum(h)
    mean = sum(v * x for v, x in enumerate(h)) / total if total else 0.0
    return dict(est_cov=est, median=median, windows=total, windows_covered=covered, windows_clamped=h[n - 1], mean=mean)


def check(hist):
    got = engine.estimate_coverage(np.asarray(hist, np.int64))
    want = restate(hist)
    for k in ("est_cov", "median", "windows", "windows_covered", "windows_clamped"):
        assert getattr(got, k) == want[k], (k, getattr(got, k), want[k])
    # mean: the library divides two sums it holds exactly, each rounded to double once (<= 0.5 ulp each), and the division rounds once
    # more; Python's int / int is correctly rounded.  Four ulps bound the difference.
    assert abs(got.mean - want["mean"]) <= 4 * 2.0 ** -52 * abs(want["mean"]), (got.mean, want["mean"])
    return got


def random_hist(rng, i):
    n = int(rng.choice([3, 4, 5, 17, 256, 4096]))
    kind = i % 4
    if kind == 0:                                   # sparse: a few bins
        h = np.zeros(n, np.int64)
        k = int(rng.integers(1, min(n, 6) + 1))
        h[rng.choice(n, k, replace=False)] = rng.integers(1, 1000, k)
    elif kind == 1:                                 # dense, small counts
        h = rng.integers(0, 50, n).astype(np.int64)
    elif kind == 2:                                 # huge counts: sums beyond 2^52 over 4096 bins, v * h beyond 2^63
        h = rng.integers(0, 1 << 40, n, dtype=np.int64)
    else:                                           # a peak with shoulders, plus mass in bin 0 and in the clamp bin
        v = np.arange(n)
        mu = float(rng.uniform(1, n - 1))
        h = (float(rng.uniform(10, 1e6)) * np.exp(-0.5 * ((v - mu) / max(mu ** 0.5, 1.0)) ** 2)).astype(np.int64)
        h[0] += int(rng.integers(0, 1 << 30))
        h[n - 1] += int(rng.integers(0, 1 << 30))
    return h


def test_random_histograms():
    rng = np.random.default_rng(20241017)
    for i in range(200):
        check(random_hist(rng, i))


@pytest.mark.parametrize("n", [3, 16, 4096])
def test_empty_and_one_sided_mass(n):
    e = check(np.zeros(n, np.int64))
    assert (e.est_cov, e.median, e.mean, e.windows) == (0, 0, 0.0, 0)
    h = np.zeros(n, np.int64); h[0] = 12345
    e = check(h)
    assert (e.est_cov, e.median, e.windows_covered, e.mean) == (0, 0, 0, 0.0)
    h = np.zeros(n, np.int64); h[n - 1] = 77
    e = check(h)
    assert (e.est_cov, e.median, e.windows_clamped) == (0, n - 1, 77)


def test_peaks_at_the_edges():
    n = 4096
    h = np.zeros(n, np.int64); h[0] = 10 ** 9; h[1] = 5; h[2] = 1
    assert check(h).est_cov == 1            # (bin 0 does not count towards s[1])
    h = np.zeros(n, np.int64); h[n - 1] = 10 ** 9; h[n - 2] = 5; h[n - 3] = 1
    assert check(h).est_cov == n - 3        # (the clamp bin does not count: s[n-3] = 0 + 1 + 5 = s[n-2] = 1 + 5 + 0, the smaller v)
    h[n - 4] = 3; h[n - 3] = 0
    assert check(h).est_cov == n - 3        # s[n-3] = 3 + 0 + 5 beats s[n-2] = 0 + 5 + 0 and s[n-4] = s[n-5] = 3
    h = np.zeros(n, np.int64); h[n - 2] = 9
    e = check(h)
    assert e.est_cov == n - 3 and e.median == n - 2      # s[n-3] = s[n-2] = 9: the smaller v


def test_tie_goes_to_the_smaller_value():
    h = np.zeros(64, np.int64); h[10] = 7; h[40] = 7
    assert check(h).est_cov == 9            # s[9] = s[10] = s[11] = s[39] = s[40] = s[41] = 7
    h = np.zeros(64, np.int64); h[9] = 1; h[10] = 5; h[11] = 1; h[39] = 2; h[40] = 5
    assert check(h).est_cov == 10           # s[10] = 7 = s[40], and s[39] = s[41] = 7 as well
    h[41] = 1
    assert check(h).est_cov == 40           # s[40] = 8


def test_three_bins():
    assert check([5, 0, 9]).est_cov == 0
    e = check([5, 3, 9])
    assert (e.est_cov, e.median, e.windows, e.windows_covered, e.windows_clamped) == (1, 2, 17, 12, 9)
    assert check([0, 9, 3]).median == 1


def test_errors():
    lib = engine.load_library()
    out = engine._CovEstimate()
    good = np.ones(8, np.int64)
    P = lambda a: C.c_void_p(a.ctypes.data)
    assert lib.raft_hip_estimate_coverage(P(good), 8, C.byref(out)) == engine.OK
    assert lib.raft_hip_estimate_coverage(P(good), 2, C.byref(out)) == engine.ERR_PARAM
    assert lib.raft_hip_estimate_coverage(P(good), 0, C.byref(out)) == engine.ERR_PARAM
    assert lib.raft_hip_estimate_coverage(P(good), -5, C.byref(out)) == engine.ERR_PARAM
    assert lib.raft_hip_estimate_coverage(None, 8, C.byref(out)) == engine.ERR_PARAM
    assert lib.raft_hip_estimate_coverage(P(good), 8, None) == engine.ERR_PARAM
    for at in (0, 3, 7):
        bad = good.copy(); bad[at] = -1
        assert lib.raft_hip_estimate_coverage(P(bad), 8, C.byref(out)) == engine.ERR_PARAM, at
    with pytest.raises(engine.RaftError) as e:
        engine.estimate_coverage([1, 2])
    assert e.value.code == engine.ERR_PARAM
    # the histogram itself needs a context: NULL is a parameter error, not a crash
    assert lib.raft_hip_cov_histogram(None, P(good), None) == engine.ERR_PARAM


def test_binding_surface():
    assert engine.COV_HIST_BINS == 4096
    assert callable(engine.Engine.coverage_histogram) and callable(engine.Engine.estimate_from)
    assert [f.name for f in dataclasses.fields(engine.CoverageEstimate)] == \
        ["est_cov", "median", "windows", "windows_covered", "windows_clamped", "mean"]
    assert {"raft_hip_cov_histogram", "raft_hip_estimate_coverage"} <= set(engine.EXPORTS)
    assert engine.Engine.last_histogram_seconds == 0.0
    # the struct's layout as the header declares it: two int32, three int64, one double
    assert C.sizeof(engine._CovEstimate) == 40
