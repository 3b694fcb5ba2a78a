"""GPU: the general bucketing's sorts (sort_pairs.hpp:101-423, bucket.hpp:353-604, engine.hip bucket_sides) at their tile, digit and
gap boundaries, against a plain reference.

Direct: every case of raft_testlib.bucket_sort_cases through Engine.group_sides -- expand_sides_kernel, radix_sort_by_key over
4096-pair tiles, unzip_sorted_kernel, fill_gaps_kernel, at any size from no side up.  The coordinate columns are tags (the slot's own
index, a hash of it), so any lost, duplicated, misplaced or re-paired side changes the output; offsets and both columns must equal
sides_reference exactly, in stable order: later digit passes are only correct if the earlier ones were stable.  One context serves a
whole group of cases, largest, smallest, second largest, ...: the ping-pong buffers and the gap list are reused in both directions.

Pass level: every set of bucket_pass_cases through run_host + finish + fetch on the three routes of bucket_sides -- window records
(radix_sort_items, 8192-item tiles, the first pass fed by SideSource), coordinate pairs (RAFT_NO_BUCKET_WINDOWS=1) and the counting
sort at any size (RAFT_NO_RADIX_SORT=1) -- against the oracle, two passes per context; and what the input can have wrong, on each
route.  tests/test_bucket_sort_cases.py shows without a GPU that the cases sit where they claim to."""
import itertools

import pytest
from raft_testlib import (PAIR_TILE, SORT_GROUPS, SORT_THRESHOLD, RaftParams, assert_same_result, assert_same_sides, bucket_pass_cases,
                          bucket_sort_cases, kernel_mode, oracle_run, sides_reference)
from test_gpu_delta4 import all_forms, result_of

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("group", SORT_GROUPS)
def test_group_sides_equals_the_reference(group):
    import torch
    from raft_amd import engine
    eng = engine.Engine(RaftParams(est_cov=1), device=0)
    try:
        for case in bucket_sort_cases(group):
            name, n_reads, cols, sym = case
            want = sides_reference(n_reads, *cols, sym)
            dev = [torch.as_tensor(c).to("cuda:0") for c in cols]
            sl = eng.group_sides(n_reads, *dev, symmetric=sym)
            assert sl.off.shape == (1, n_reads + 1), name
            got = (sl.off[0], sl.qs.cpu().numpy(), sl.qe.cpu().numpy())
            assert_same_sides(name, n_reads, cols, sym, got, want, PAIR_TILE)
    finally:
        eng.close()


# ---- pass level ------------------------------------------------------------------------------------------------------------------------

ROUTES = {"windows": {}, "pairs": {"RAFT_NO_BUCKET_WINDOWS": "1"}, "counting": {"RAFT_NO_RADIX_SORT": "1"}}
PASS_CASES = {c.name: c for c in bucket_pass_cases()}
_held = {}


def pass_set(name):
    """(case, params, columns, the oracle's result) -- made once per set (the items of a set follow each other) and left unchanged."""
    if _held.get("name") != name:
        _held.clear()
        case = PASS_CASES[name]
        p, cols = case.build()
        _held.update(name=name, value=(case, p, cols, oracle_run(p, *cols)))
    return _held["value"]


def set_route(monkeypatch, route):
    for k in ("RAFT_NO_BUCKET_WINDOWS", "RAFT_NO_RADIX_SORT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)


def one_pass(eng, cols):
    eng.run_host(*cols)
    s = eng.finish()
    return result_of(eng, s), s


def check_pass(eng, case, cols, want, route, what):
    """One pass over `cols`: the oracle's arrays, the general bucketing, its interval count, the route the pass says it took."""
    from raft_amd import engine
    got, s = one_pass(eng, cols)
    assert_same_result(got, want, what)
    qid, tid = cols[1], cols[4]
    n = qid.size
    cap_iv = n if case.symmetric else 2 * n
    assert s.interval_path == 1, (what, s.interval_path)
    assert s.n_intervals == (n if case.symmetric else n + int((qid != tid).sum())) == want["n_intervals"], (what, s.n_intervals)
    # (a set with a side beyond 16 bits of windows cannot go as window records: the pass is run again with coordinate pairs)
    windows = route == "windows" and cap_iv >= SORT_THRESHOLD and not case.wide
    assert bool(s.flags & engine.SUM_BUCKET_WINDOWS) == windows, (what, s.flags, cap_iv)
    return s


@pytest.mark.parametrize("name,route", list(itertools.product(PASS_CASES, ROUTES)))
def test_pass_equals_oracle_on_every_route(name, route, monkeypatch):
    from raft_amd import engine
    case, p, cols, want = pass_set(name)
    set_route(monkeypatch, route)
    eng = engine.Engine(p, device=0)
    try:
        for rep in range(2):
            s = check_pass(eng, case, cols, want, route, f"set {name}, route {route}, pass {rep}")
            if name == "edge16_fits":
                assert not s.flags & engine.SUM_RERUN, (route, rep, s.flags)
            if name == "edge16_wide":       # kErrWide once: this context buckets coordinate pairs from then on
                assert bool(s.flags & engine.SUM_RERUN) == (route == "windows" and rep == 0), (route, rep, s.flags)
    finally:
        eng.close()


@pytest.mark.parametrize("name,form", list(itertools.product(("thr_at", "gaps"), ("deep", "width 8"))))
def test_pass_through_the_deep_kernel_and_the_step_encoding(name, form, monkeypatch):
    from raft_amd import engine
    case, p, cols, want = pass_set(name)
    set_route(monkeypatch, "windows")
    eng = engine.Engine(p, device=0)
    try:
        if form == "deep":
            with kernel_mode("deep"):
                for rep in range(2):
                    check_pass(eng, case, cols, want, "windows", f"set {name}, deep kernel, pass {rep}")
        else:
            def run():
                eng.run_host(*cols)
                return eng.finish()
            all_forms(eng, run, want, f"set {name}, window records", direct=False)
    finally:
        eng.close()


@pytest.mark.parametrize("route", list(ROUTES))
def test_errors_on_every_route(route, monkeypatch):
    """tiles257 with ids out of range (the first such record is named whichever side it is on), coordinates of a side that does not exist
    (ignored, as by the oracle), a negative coordinate of one that does; the context is itself again after each."""
    from raft_amd import engine
    case, p, cols, want = pass_set("tiles257")
    set_route(monkeypatch, route)
    rl, qid, qs, qe, tid, ts, te = cols
    n_reads = rl.size
    eng = engine.Engine(p, device=0)

    def clean(what):
        check_pass(eng, case, cols, want, route, f"tiles257, route {route}, {what}")

    def fails(c):
        with pytest.raises(engine.RaftError) as e:
            eng.run_host(*c)
            eng.finish()
        return e.value
    try:
        clean("first pass")
        for first, second in ((4, 1), (1, 4)):                    # (column 4: tid, 1: qid)
            bad = [c.copy() for c in cols]
            bad[first][17] = n_reads + 5
            bad[second][300000] = -1 if second == 1 else n_reads
            err = fails(bad)
            assert err.code == engine.ERR_READ_ID and err.index == 17, (route, first, err.code, err.index)
            clean(f"after a bad id in column {first}")
        # a target side on the query's own read does not exist: its coordinates are never looked at (chop.hpp:166)
        i = 123456
        odd = [c.copy() for c in cols]
        odd[4][i] = odd[1][i]
        odd[5][i], odd[6][i] = -7, int(rl[odd[1][i]]) + 10 ** 6
        want_odd = oracle_run(p, *odd)
        got, s = one_pass(eng, odd)
        assert_same_result(got, want_odd, f"tiles257, route {route}, coordinates of a side that does not exist")
        assert s.n_intervals == want_odd["n_intervals"]
        clean("after a self overlap with wild target coordinates")
        neg = [c.copy() for c in cols]
        neg[2][999] = -3
        assert fails(neg).code == engine.ERR_COORD                # (the index depends on the route: include/raft_hip.h)
        clean("after a negative coordinate")
    finally:
        eng.close()
