"""GPU: raft_hip_repeat_stats_device / _host (raft_amd/csrc/repeat_stats.hpp, libraft_hip_rst.so) -- per repeat run the overlap sides
that touch it, span it and lie inside it, the coverage over its windows, its flags, the summary -- exact against the brute-force model
(tests/test_repeat_stats_cases.py repeat_stats_model): at every unit boundary of the record kernel (lane, wave, workgroup), on both load
paths, in both forms, under symmetric 0 and 1; streaks of one single-run read across those boundaries in either column, one of them
past 16 bits; runs of every window count around a lane's, a step's and two steps' windows at every alignment of the first window; the
coverage part after passes of every output width; one context over sizes going up and down; every error; the golden fixtures with the
context's own pass."""
import ctypes as C

import numpy as np
import pytest
from raft_testlib import assert_same_result, oracle_run
from test_gpu_repeat_overlaps import on_device
from test_repeat_overlaps_cases import GOLDEN_ANCHORS, golden_case, golden_params
from test_repeat_stats_cases import (ARRAYS, AT_END, COUNTS, COVERAGE, STREAKS, SUMMARY, case_reads, census, csr, i32, lattice_case, repeat_stats_model,
                                     same_stats, stream, streak_case)

from raft_amd.params import RaftParams

pytestmark = pytest.mark.gpu
WIDTHS = (4, 2, 1, 8)          # int32, uint16 codes, byte codes, four-bit steps (RAFT_HIP_COV_DELTA4)
RECORD_COUNTS = (0, 1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2049)
WINDOW_COUNTS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 513)
RESO = 50


@pytest.fixture(scope="module")
def eng():
    from raft_amd import engine
    e = engine.Engine(RaftParams(est_cov=30), device=0)
    yield e
    e.close()


def check(eng, cols, sym, rep, what, forms=("host", "device"), want=None, shift=0, **cov):
    """Without coverage (threshold 0) unless cov = dict(threshold, cov_offset, cov, reso) of the context's finished pass."""
    thr = cov.get("threshold", 0)
    if want is None:
        want = repeat_stats_model(*cols, sym, *rep, **cov)
    for form in forms:
        if form == "host":
            got = eng.repeat_stats(*cols, symmetric=sym, repeats=rep, threshold=thr)
        else:
            got = eng.repeat_stats(*on_device(cols, shift), symmetric=sym, repeats=on_device(rep), threshold=thr)
        same_stats(got, want, f"{what}, {form} form, symmetric {int(sym)}")
        assert eng.last_repeat_stats_seconds >= 0.0
        assert (got["run_span"] <= got["run_touch"]).all() and (got["run_inside"] <= got["run_touch"]).all()
    return want


# ---- the record kernel's units ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_rec", RECORD_COUNTS)
def test_record_counts(eng, n_rec):
    cols, rep = stream(n_rec)
    for sym in (False, True):
        want = check(eng, cols, sym, rep, f"{n_rec} records")
        if n_rec >= 1023:
            seen = census(cols, sym, rep, want)
            assert all(seen[k] > 0 for k in ("touch_only", "span_not_inside", "inside_not_span", "all_three", "walk_breaks_early", "walk_reaches_last_run")), seen


@pytest.mark.parametrize("n_rec", (1, 5, 257, 1025))
def test_columns_offset_by_one_element(eng, n_rec):
    """No column is 16-byte aligned: the 4-byte load path, the same numbers."""
    cols, rep = stream(n_rec, seed=9)
    for sym in (False, True):
        check(eng, cols, sym, rep, f"{n_rec} records, shifted", forms=("device",), shift=1)


@pytest.mark.parametrize("sym", (False, True))
def test_the_lattice_around_every_run(eng, sym):
    cols, rep = lattice_case()
    check(eng, cols, sym, rep, "lattice")
    check(eng, cols[:5] + [None, None], True, rep, "lattice, no target columns", forms=("host",))


@pytest.mark.parametrize("column", ("q", "t"))
@pytest.mark.parametrize("n", STREAKS)
def test_streaks_of_one_single_run_read(eng, n, column):
    """The join within the lane, across the wave, and its end at a wave's and a workgroup's edge: the streak begins 0 .. 3 records into
    its first lane."""
    for lead in ((3,) if n >= 70000 else (0, 1, 2, 3)):
        cols, rep = streak_case(n, column, lead)
        want = check(eng, cols, False, rep, f"a streak of {n} in the {column} column behind {lead}", forms=("device",) if lead else ("host", "device"))
        assert want["run_touch"][0] == n
        if n >= 70000:
            assert want["run_span"][0] == want["run_inside"][0] == n > 1 << 16


def test_no_reads_no_records_no_runs(eng):
    e = np.empty(0, np.int32)
    z = np.zeros(1, np.int64)
    check(eng, [e] * 7, False, (z, e, e), "no reads")
    cols, rep = stream(5)
    for sym in (False, True):
        check(eng, [cols[0]] + [e] * 6, sym, rep, "no records")
        check(eng, [cols[0]] + [None] * 6, sym, rep, "records NULL", forms=("host",))
    check(eng, cols, False, (np.zeros(cols[0].size + 1, np.int64), e, e), "no runs")


def test_sizes_going_up_and_down_on_one_context(eng):
    for n_rec in (1025, 5, 20001, 3, 0, 257):
        cols, rep = stream(n_rec, seed=2)
        check(eng, cols, False, rep, f"{n_rec} records")
        if n_rec % 2:
            many = [case_reads()[1][4]] * (n_rec % 7 + 1) + [[]]                  # ... and another annotation: 130 runs a read
            lens = i32(*[30000] * len(many))
            c2 = [lens] + [c % len(many) if k in (0, 3) else c for k, c in enumerate(cols[1:])]
            check(eng, c2, False, csr(many), f"{n_rec} records on {len(many)} reads")


# ---- the coverage part ---------------------------------------------------------------------------------------------------------------------

def window_set():
    """Reads for a pass: one of 900 windows, one of 7 whose length is no multiple of the window, one piled 320 deep on its first windows
    (the one-byte form lists them), one of one window, a read of length 0, and some more, with a few self overlaps each."""
    from test_read_stats_cases import overlaps_for
    cols = overlaps_for([900, 7, 600, 1, 0, 33, 64, 257], 4, reso=RESO)
    cols[0][1] = 7 * RESO - 13
    for k in (2, 3, 5, 6):
        cols[k] = np.minimum(cols[k], cols[0][cols[1]])
    deep = np.full(320, 2, np.int32)
    add = [deep, np.zeros(320, np.int32), np.full(320, 4 * RESO - 1, np.int32)]
    return [cols[0]] + [np.concatenate([cols[k], add[(k - 1) % 3]]).astype(np.int32) for k in range(1, 7)]


def window_runs(lens, cov_offset):
    """Explicit runs over the pass's windows: every count of WINDOW_COUNTS at the four alignments of the first window's index in the
    coverage array, runs whose ends lie on and one off a window edge, a run ending at the read's end, one reaching behind it, one before
    its start, an EMPTY one.  rep_s ascends within a read."""
    runs = [[] for _ in lens]
    for m in range(4):
        j0 = 3 + (m - int(cov_offset[0]) - 3) % 4
        assert (int(cov_offset[0]) + j0) % 4 == m
        runs[0] += [(j0 * RESO, (j0 + n) * RESO) for n in WINDOW_COUNTS]
        j0 = (m - int(cov_offset[2])) % 4
        runs[2] += [(j0 * RESO, (j0 + n) * RESO) for n in (1, 2, 300)]            # (the deep windows of read 2 among them)
    runs[0] += [(20 * RESO + da, 30 * RESO + db) for da in (-1, 0, 1) for db in (-1, 0, 1)]
    L1 = int(lens[1])
    runs[1] = [(-40, 60), (0, L1), (RESO, L1), (2 * RESO + 1, L1 + 200), (L1 - 1, L1), (L1, L1 + 50), (L1 + 60, L1 + 400)]
    runs[3] = [(0, int(lens[3])), (10, 10)]
    runs[4] = [(0, 10)]                                                           # (a read of length 0 has no window)
    runs[5] = [(0, 1), (RESO - 1, RESO), (RESO - 1, RESO + 1), (RESO, RESO + 1)]
    runs[7] = [(0, int(lens[7]))]
    return csr([sorted(r, key=lambda x: x[0]) for r in runs])


@pytest.mark.parametrize("width", WIDTHS)
def test_coverage_windows_in_every_form(width):
    from raft_amd import engine
    cols = window_set()
    p = RaftParams(reso=RESO, est_cov=4, symmetric_mode=1)
    eng = engine.Engine(p, device=0)
    try:
        eng.set_output_width(width)
        eng.run_host(*cols)
        s = eng.finish()
        cov_offset = np.concatenate([[0], np.cumsum(-(-cols[0].astype(np.int64) // RESO))])
        rep = window_runs(cols[0], cov_offset)
        first = {form: eng.repeat_stats(*(cols if form == "host" else on_device(cols)), symmetric=True, repeats=rep if form == "host" else on_device(rep),
                                        threshold=5) for form in ("host", "device")}          # (before anybody fetched: the pass's own form is read)
        got = eng.fetch()
        assert np.array_equal(got["cov_offset"], cov_offset) and got["cov"].dtype == np.int32
        cov = dict(threshold=5, cov_offset=cov_offset, cov=got["cov"], reso=RESO)
        want = repeat_stats_model(*cols, True, *rep, **cov)
        for form, g in first.items():
            same_stats(g, want, f"width {width}, {form} form, before the fetch")
        check(eng, cols, True, rep, f"width {width}, after the fetch", **cov)
        k = int(rep[0][2])
        assert want["run_cov_max"][k:rep[0][3]].max() >= 300 and set(WINDOW_COUNTS) <= set(want["run_windows"].tolist())
        firsts = (cov_offset[np.repeat(np.arange(len(cols[0])), np.diff(rep[0]))] + np.maximum(rep[1], 0) // RESO) % 4
        for n in WINDOW_COUNTS:
            assert set(firsts[want["run_windows"] == n].tolist()) == {0, 1, 2, 3}, n
        assert (want["run_windows"] == 0).sum() >= 3 and (want["run_flags"] & AT_END != 0).any()
        # another threshold, the counts untouched; the context's own annotation and its high_cov by default
        check(eng, cols, True, rep, f"width {width}, threshold 1", forms=("device",), **dict(cov, threshold=1))
        own = (got["rep_offset"], got["rep_s"], got["rep_e"])
        same_stats(eng.repeat_stats(*cols, symmetric=True), repeat_stats_model(*cols, True, *own, **dict(cov, threshold=p.high_cov)), "own annotation")
        assert_same_result(dict(eng.fetch(), symmetric=s.symmetric, high_cov=s.high_cov, total_coverage=s.total_coverage, total_windows=s.total_windows,
                                total_repeat_length=s.total_repeat_length, total_read_length=s.total_read_length),
                           oracle_run(p, *cols) | {"symmetric": 1}, f"width {width}: the pass after the calls")
    finally:
        eng.close()


# ---- the ABI: errors, NULL outputs ----------------------------------------------------------------------------------------------------------

OUTPUTS = ARRAYS + ("sum", "err")
OWN = "own"


def raw(eng, form, cols, sym, rep, threshold=0, skip=COVERAGE, n_reads=None, n_rec=None, n_rep=None, rows=None):
    """The entry point as the ABI has it; outputs filled with a mark before the call.  rep: three arrays (None = NULL) or OWN.
    -> rc, error_index, {name: array}, summary"""
    from raft_amd import engine
    lib = engine.load_side_library("rst")
    if n_rep is None:
        n_rep = -1 if rep == OWN else 0 if rep[1] is None else rep[1].size
    rows = (max(n_rep, 0) if rep != OWN else int(eng.summary.n_repeats)) if rows is None else rows
    rep = [None] * 3 if rep == OWN else list(rep)
    n_reads = cols[0].size if n_reads is None else n_reads
    n_rec = next((c.size for c in cols[1:] if c is not None), 0) if n_rec is None else n_rec
    out = {k: np.full(min(rows, 1 << 20), -7, np.int64 if k == "run_cov_sum" else np.int32) for k in ARRAYS}
    out["run_flags"] = np.full(min(rows, 1 << 20), 249, np.uint8)
    sm, err = engine._RstSummary(), C.c_int64(-5)
    sm.n_runs = -9
    if form == "device":
        import torch
        dcols, drep = on_device(cols), on_device(rep)
        A = lambda t: 0 if t is None else t.data_ptr()
        eng.use_torch_stream()
        fn = lib.raft_hip_repeat_stats_device
    else:
        keep = lambda xs: [None if a is None else np.ascontiguousarray(a) for a in xs]
        dcols, drep = keep(cols), keep(rep)
        A = lambda a: 0 if a is None else a.ctypes.data
        fn = lib.raft_hip_repeat_stats_host
    records = engine._Records(n_rec, *[A(c) for c in dcols[1:]])
    names = dict(zip(OUTPUTS, [C.c_void_p(out[k].ctypes.data) for k in ARRAYS] + [C.byref(sm), C.byref(err)]))
    outs = [None if k in skip else v for k, v in names.items()]
    rc = fn(eng._ctx, n_reads, C.c_void_p(A(dcols[0])), C.byref(records), int(sym), n_rep, *[C.c_void_p(A(a)) for a in drep], threshold, *outs, None)
    if form == "device":
        torch.cuda.synchronize()
    return rc, err.value, out, sm


def untouched(out, sm):
    return all((a == (249 if a.dtype == np.uint8 else -7)).all() for a in out.values()) and sm.n_runs == -9


@pytest.mark.parametrize("form", ("host", "device"))
def test_an_id_out_of_range_names_the_first_record(eng, form):
    from raft_amd import engine
    cols, rep = stream(5000)
    n_reads = cols[0].size
    for bad_at in (((1, 4203, n_reads), (4, 1203, -1), (1, 2210, -3)), ((4, 0, n_reads + 7), (1, 4999, -1)), ((1, 4999, n_reads), (4, 4999, -2)),
                   ((4, 3071, 2**31 - 1), (1, 3072, -2**31))):
        bad = [c.copy() for c in cols]
        for col, at, value in bad_at:
            bad[col][at] = value
        for sym in (False, True):
            rc, err, out, sm = raw(eng, form, bad, sym, rep)
            assert rc == engine.ERR_READ_ID and err == min(at for _, at, _ in bad_at), (bad_at, rc, err)
            assert untouched(out, sm), bad_at
    e = np.empty(0, np.int32)
    rc, err, out, sm = raw(eng, form, bad, False, (np.zeros(n_reads + 1, np.int64), e, e))         # without a run the ids are checked too
    assert rc == engine.ERR_READ_ID and err == 3071
    rc, err, out, sm = raw(eng, form, cols, False, rep)
    assert rc == 0 and err == -1 and not untouched(out, sm)


def _violations(rep):
    off, s, e = rep
    with_runs = int(np.flatnonzero(np.diff(off) > 1)[1])

    def edit(k, value):
        out = off.copy(); out[k] = value
        return (out, s, e)
    yield "first offset not 0", edit(0, 1), {}
    yield "offsets step back", edit(with_runs + 1, off[with_runs] - 1), {}
    yield "an offset negative", edit(1, -1), {}
    yield "an offset beyond the arrays", edit(with_runs, off[-1] + 5), {}
    yield "last offset short of n_rep", edit(len(off) - 1, off[-1] - 1), {}
    yield "last offset beyond the arrays", edit(len(off) - 1, off[-1] + 1), {}
    yield "n_rep not the last offset", rep, {"n_rep": s.size - 1}
    yield "no rep_offset", (None, s, e), {}
    yield "no rep_s", (off, None, e), {"n_rep": e.size}
    yield "no rep_e", (off, s, None), {}
    yield "arrays but n_rep = -1", rep, {"n_rep": -1, "rows": s.size}
    yield "n_rep = -2", rep, {"n_rep": -2}
    yield "n_rec = -1", rep, {"n_rec": -1}
    yield "n_reads = -1", rep, {"n_reads": -1}
    yield "threshold = -1", rep, {"threshold": -1}


@pytest.mark.parametrize("form", ("host", "device"))
def test_bad_arguments(eng, form):
    from raft_amd import engine
    cols, rep = stream(300)
    seen = 0
    for what, bad_rep, kw in _violations(rep):
        rc, err, out, sm = raw(eng, form, cols, False, bad_rep, **kw)
        assert rc == engine.ERR_PARAM, (what, rc)
        assert untouched(out, sm), what
        seen += 1
    assert seen == 15
    for k in range(1, 7):                                              # a missing column; ts / te may both be missing under symmetric
        for sym in (False, True):
            rc, err, out, sm = raw(eng, form, cols[:k] + [None] + cols[k + 1:], sym, rep)
            assert rc == engine.ERR_PARAM and untouched(out, sm), (k, sym)
    rc, err, out, sm = raw(eng, form, cols[:5] + [None, None], False, rep)
    assert rc == engine.ERR_PARAM and untouched(out, sm)
    rc, err, out, sm = raw(eng, form, cols[:5] + [None, None], True, rep)
    assert rc == 0 and np.array_equal(out["run_touch"], repeat_stats_model(*cols, True, *rep)["run_touch"])
    for kw in ({"n_rec": 2**30}, {"n_rep": 2**31 - 1, "rows": 8}):      # (refused before anything is read)
        rc, err, out, sm = raw(eng, form, cols, False, rep, **kw)
        assert rc == engine.ERR_TOO_LARGE and untouched(out, sm), kw
    for name in COVERAGE:                                              # threshold 0 with a coverage output
        rc, err, out, sm = raw(eng, form, cols, False, rep, skip=tuple(k for k in COVERAGE if k != name))
        assert rc == engine.ERR_PARAM and untouched(out, sm), name
    rc, err, out, sm = raw(eng, form, cols, False, rep)                # ... and the context is as good as before
    assert rc == 0 and not untouched(out, sm)
    with pytest.raises(ValueError):                                    # (offsets of another number of reads: refused before the library reads them)
        eng.repeat_stats(*cols, repeats=(rep[0][:-1], rep[1], rep[2]), threshold=0)


@pytest.mark.parametrize("form", ("host", "device"))
def test_every_output_null_in_turn(form):
    from raft_amd import engine
    cols = window_set()
    eng = engine.Engine(RaftParams(reso=RESO, est_cov=4, symmetric_mode=1), device=0)
    try:
        eng.run_host(*cols)
        eng.finish()
        got = eng.fetch()
        rep = window_runs(cols[0], got["cov_offset"])
        want = repeat_stats_model(*cols, True, *rep, threshold=3, cov_offset=got["cov_offset"], cov=got["cov"], reso=RESO)
        for skip in OUTPUTS + (OUTPUTS, COUNTS, COVERAGE):
            skip = (skip,) if isinstance(skip, str) else skip
            rc, err, out, sm = raw(eng, form, cols, True, rep, threshold=3, skip=skip)
            assert rc == 0, skip
            for name in ARRAYS:
                assert (out[name] == (249 if name == "run_flags" else -7)).all() if name in skip else np.array_equal(out[name], want[name]), (skip, name)
            assert sm.n_runs == (-9 if "sum" in skip else rep[1].size) and err == (-5 if "err" in skip else -1)
            if "sum" not in skip:
                assert all(getattr(sm, k) == want[k] for k in SUMMARY)
    finally:
        eng.close()


def test_the_states_of_the_context():
    from raft_amd import engine
    from test_read_stats_cases import overlaps_for
    p = RaftParams(est_cov=3, symmetric_mode=1)
    cols = overlaps_for([500, 77, 1200] * 5, 3)
    n_reads = len(cols[0])
    one_each = (np.arange(n_reads + 1, dtype=np.int64), np.full(n_reads, 100, np.int32), (np.asarray(cols[0]) - 100).astype(np.int32))
    eng = engine.Engine(p, device=0)

    def state_error():
        for kw in ({}, {"threshold": 0}, {"repeats": one_each}, {"repeats": one_each, "threshold": 2}):
            with pytest.raises(engine.RaftError) as ex:
                eng.repeat_stats(*cols, symmetric=True, **kw)
            assert ex.value.code == engine.ERR_STATE, kw
        got = eng.repeat_stats(*cols, symmetric=True, repeats=one_each, threshold=0)                # explicit arrays, no coverage: any state
        same_stats(got, repeat_stats_model(*cols, True, *one_each), "explicit arrays")

    state_error()                                                   # no pass at all
    eng.run_host(*cols)
    eng.finish()
    f = eng.fetch()
    rep, cov = (f["rep_offset"], f["rep_s"], f["rep_e"]), dict(cov_offset=f["cov_offset"], cov=f["cov"], reso=p.reso)
    same_stats(eng.repeat_stats(*cols, symmetric=True), repeat_stats_model(*cols, True, *rep, threshold=p.high_cov, **cov), "after finish")
    same_stats(eng.repeat_stats(*cols, symmetric=True, repeats=one_each, threshold=2), repeat_stats_model(*cols, True, *one_each, threshold=2, **cov), "explicit")
    for kw in ({}, {"repeats": (one_each[0][:-1], one_each[1][:-1], one_each[2][:-1])}, {"threshold": 0}):
        with pytest.raises(engine.RaftError) as ex:                  # n_reads is not the pass's
            eng.repeat_stats(cols[0][:-1], *[c[cols[1] < n_reads - 1] for c in cols[1:]], symmetric=True, **kw)
        assert ex.value.code == engine.ERR_PARAM, kw
    eng.run_pipelined(*cols[:4], n_chunks=3)                        # host to host: the context holds no pass afterwards
    state_error()
    eng.run_host(*cols)
    eng.finish()
    same_stats(eng.repeat_stats(*cols, symmetric=True), repeat_stats_model(*cols, True, *rep, threshold=p.high_cov, **cov), "after the pipeline")
    eng.close()


def test_the_call_hands_out_no_geometry():
    """After a speculated pass the own-pass call answers as after any other, and the pass behind it is speculated on kept geometry."""
    import torch
    from raft_amd import engine
    from test_gpu_speculate import _set
    p = RaftParams(est_cov=4, repeat_length=2000, interval_length=2000, symmetric_mode=1)
    rl, (qid, a, b) = _set(31)
    cols = [rl, qid, a, b, qid, a, b]
    want_pass = oracle_run(p, *cols); want_pass["symmetric"] = 1      # (asserted by the parameters, not detected)
    rep = (want_pass["rep_offset"], want_pass["rep_s"], want_pass["rep_e"])
    want = repeat_stats_model(*cols, True, *rep, threshold=p.high_cov, cov_offset=want_pass["cov_offset"], cov=want_pass["cov"], reso=p.reso)
    assert want["runs_spanned"] > 0 and want["sides_inside"] > 0 and (np.diff(rep[0]) > 1).any()
    dev = [torch.from_numpy(x).to("cuda:0") for x in (rl, qid, a, b)]
    eng = engine.Engine(p, device=0)
    for it in range(2):
        eng.run_device(*dev); s = eng.finish()
    assert s.flags & engine.SUM_SPECULATED
    same_stats(eng.repeat_stats(*on_device(cols), symmetric=True), want, "after a speculated pass, device form")
    same_stats(eng.repeat_stats(*cols, symmetric=True), want, "after a speculated pass, host form")
    eng.run_device(*dev); s = eng.finish()
    assert s.flags & engine.SUM_SPECULATED and s.flags & engine.SUM_KEPT_GEOMETRY, s.flags
    got = eng.fetch()
    got.update(symmetric=s.symmetric, high_cov=s.high_cov, total_coverage=s.total_coverage, total_windows=s.total_windows,
               total_repeat_length=s.total_repeat_length, total_read_length=s.total_read_length)
    assert_same_result(got, want_pass, "the speculated pass behind the call")
    eng.close()


# ---- the goldens ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(GOLDEN_ANCHORS))
def test_golden_fixtures_with_the_own_pass(name):
    from raft_amd import engine
    cols, ref_rep = golden_case(name)
    p = RaftParams(**golden_params(name))
    eng = engine.Engine(p, device=0)
    try:
        eng.run_host(*cols)
        s = eng.finish()
        sym = bool(s.symmetric)
        got = {"host": eng.repeat_stats(*cols, symmetric=sym), "device": eng.repeat_stats(*on_device(cols), symmetric=sym)}
        stats = eng.read_stats()
        f = eng.fetch()
        rep = (f["rep_offset"], f["rep_s"], f["rep_e"])
        for a, b in zip(rep, ref_rep):
            assert np.array_equal(a, b), name
        want = repeat_stats_model(*cols, sym, *rep, threshold=p.high_cov, cov_offset=f["cov_offset"], cov=f["cov"], reso=p.reso)
        for form, g in got.items():
            same_stats(g, want, f"{name}, {form} form")
        g = got["device"]
        assert g["n_runs"] > 0 and g["runs_spanned"] > 0 and g["sides_inside"] > 0
        read = np.repeat(np.arange(len(cols[0])), np.diff(rep[0]))
        have = g["run_windows"] > 0
        assert have.all()                                              # (the engine's runs lie inside their reads)
        assert (g["run_cov_min"][have] >= g["run_span"][have]).all(), name          # a spanning side covers every window of the run
        assert (g["run_cov_max"] <= stats["cov_max"][read]).all(), name
        assert (g["run_high"] > 0).all() and (g["run_cov_max"] >= p.high_cov).all(), name       # a repeat holds high windows
        whole = np.flatnonzero((np.diff(rep[0])[read] == 1) & (rep[1] == 0) & (rep[2] == cols[0][read]))
        assert np.array_equal(g["run_cov_sum"][whole], stats["cov_sum"][read[whole]]), name
        # the same counts without the coverage part
        same_stats(eng.repeat_stats(*cols, symmetric=sym, threshold=0), repeat_stats_model(*cols, sym, *rep), f"{name}, threshold 0")
    finally:
        eng.close()
