"""GPU: raft_hip_frag_overlaps_device / _host (raft_amd/csrc/frag_ovl.hpp, libraft_hip_frag.so) -- per fragment the overlap sides that
touch, span and contain it, its bases inside repeats, per read its contained fragments, the summary -- exact against the definitions
restated in numpy (tests/test_fragment_overlaps_cases.py want_fragments): at every unit boundary of the record kernel (lane, wave,
workgroup, one turn of the grid-stride loop) and of the scan (tile, one turn of its loop over the tiles before), on both load paths, in
both forms, under symmetric 0 and 1, on reads of 1 to 1000 rows with sides on every row boundary, with every side of several workgroups
on one read, on the hand-written cases with their literal numbers, on the golden fixtures with the reference's fragment and repeat
arrays, against a context's own finished pass in every output width, and in every state of the context."""
import ctypes as C

import numpy as np
import pytest
from raft_testlib import assert_same_result, oracle_run
from test_fragment_overlaps_cases import (ARRAYS, COUNTS, GOLDENS, HAND, HOT_COUNTS, ROW_COUNTS, SUMMARY, TABLE_SIZES, big_table, classes, golden_case,
                                          hand_case, hot_read, one_read, same_fragments, stream, want_fragments)
from test_gpu_repeat_overlaps import on_device
from test_repeat_overlaps_cases import golden_params

from raft_amd.params import RaftParams

pytestmark = pytest.mark.gpu
WIDTHS = (4, 1, 2, 8)          # int32, byte codes, uint16 codes, four-bit steps (RAFT_HIP_COV_DELTA4)


@pytest.fixture(scope="module")
def eng():
    from raft_amd import engine
    e = engine.Engine(RaftParams(est_cov=30), device=0)
    yield e
    e.close()


def check(eng, cols, sym, table, rep, what, forms=("host", "device"), want=None, shift=0):
    """rep: (rep_offset, rep_s, rep_e), or () for no annotation."""
    if want is None:
        want = want_fragments(*cols, sym, *table, *rep)
    for form in forms:
        if form == "host":
            got = eng.fragment_overlaps(*cols, symmetric=sym, fragments=table, repeats=rep)
        else:
            got = eng.fragment_overlaps(*on_device(cols, shift), symmetric=sym, fragments=on_device(table), repeats=on_device(rep))
            assert all(got[k].is_cuda for k in ARRAYS[:4])
        same_fragments(got, want, f"{what}, {form} form, symmetric {int(sym)}")
        assert eng.last_fragment_overlaps_seconds >= 0.0
        # the summary is the sums of the arrays
        a = {k: (got[k].cpu().numpy() if hasattr(got[k], "is_cuda") else got[k]) for k in ARRAYS}
        rows = np.diff(table[0])
        assert got["n_records"] == cols[1].size and got["n_fragments"] == a["frag_touch"].size == rows.sum()
        assert got["frags_untouched"] == int((a["frag_touch"] == 0).sum()) and got["frags_spanned"] == int((a["frag_span"] > 0).sum())
        assert got["frags_contained"] == int((a["frag_contained"] > 0).sum())
        assert got["frags_contained_repeat"] == int(((a["frag_contained"] > 0) & (a["frag_repeat"] > 0)).sum())
        assert got["reads_any_contained"] == int((a["read_contained"] > 0).sum())
        assert got["reads_all_contained"] == int(((rows > 0) & (a["read_contained"] == rows)).sum())
        assert (a["frag_contained"] <= a["frag_span"]).all() and (a["frag_span"] <= a["frag_touch"]).all()
    return want


# ---- the record kernel's units ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_rec", COUNTS)
def test_record_counts(eng, n_rec):
    cols, table, rep = stream(n_rec)
    big = n_rec > 100000           # (one turn of the grid-stride loop: the model once, both forms)
    want = check(eng, cols, False, table, rep, f"{n_rec} records")
    if n_rec >= 1023:
        seen = classes(want, table)
        assert all(seen.values()), seen
    if not big:
        check(eng, cols, True, table, rep, f"{n_rec} records")


@pytest.mark.parametrize("n_rec", (1, 5, 257, 1025))
def test_columns_offset_by_one_element(eng, n_rec):
    """No column is 16-byte aligned: the 4-byte load path, the same numbers."""
    cols, table, rep = stream(n_rec, seed=9)
    for sym in (False, True):
        check(eng, cols, sym, table, rep, f"{n_rec} records, shifted", forms=("device",), shift=1)


@pytest.mark.parametrize("n_rows", ROW_COUNTS)
def test_one_read_with_sides_on_every_row_boundary(eng, n_rows):
    cols, table, rep = one_read(n_rows)
    for sym in (False, True):
        want = check(eng, cols, sym, table, rep, f"one read of {n_rows} rows")
        assert want["frag_span"][:n_rows].min() > 0 and want["frag_contained"][:n_rows].min() > 0
        assert (want["frag_span"] > want["frag_contained"]).any() and (want["frag_touch"] > want["frag_span"]).any()


@pytest.mark.parametrize("n_frag", TABLE_SIZES)
def test_table_sizes_around_the_scan_units(eng, n_frag):
    cols, table = big_table(n_frag)
    want = check(eng, cols, False, table, (), f"{n_frag} rows")
    if n_frag > 1:
        assert want["frags_contained"] > 0 and want["frags_untouched"] > 0 and want["frag_touch"][-1] > 0 and want["frag_touch"][0] > 0
        check(eng, cols, True, table, (), f"{n_frag} rows", forms=("device",), want=want_fragments(*cols, True, *table))


@pytest.mark.parametrize("n_rec", HOT_COUNTS)
def test_every_side_on_one_read(eng, n_rec):
    """Every side of one workgroup, and of several, adds to the same few slots."""
    cols, table = hot_read(n_rec)
    for sym in (False, True):
        want = check(eng, cols, sym, table, (), f"{n_rec} records on one read")
        assert want["frag_touch"][:3].min() > n_rec // 4 and want["frag_contained"][:3].min() > 0


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_written_cases(eng, name):
    cols, sym, table, rep, exp = hand_case(name)
    want = check(eng, cols, sym, table, rep, name)
    for k, v in exp.items():
        assert np.array_equal(want[k], v), (name, k)
    check(eng, cols, sym, table, (), name + ", no annotation")


def test_no_reads_no_records_no_rows(eng):
    e = np.empty(0, np.int32)
    check(eng, [e] * 7, False, (np.zeros(1, np.int64), e, e), (), "no reads")
    check(eng, [e] * 7, False, (np.zeros(1, np.int64), e, e), (np.zeros(1, np.int64), e, e), "no reads, an empty annotation")
    cols, table, rep = stream(5)
    for sym in (False, True):
        check(eng, [cols[0]] + [e] * 6, sym, table, rep, "no records")
    check(eng, cols, False, (np.zeros(cols[0].size + 1, np.int64), e, e), rep, "no rows")


def test_sizes_going_up_and_down_on_one_context(eng):
    for n_rec, n_frag in ((1025, 4097), (5, 1), (70001, 0), (3, 2049), (0, 4097), (257, 7)):
        cols, table = big_table(n_frag, n_rec=n_rec)
        check(eng, cols, False, table, (), f"{n_rec} records on {n_frag} rows")
    for n_rec in (1023, 4, 20000):
        cols, table, rep = stream(n_rec, seed=2)
        check(eng, cols, False, table, rep, f"{n_rec} records after the others")


# ---- the ABI: errors, NULL outputs ----------------------------------------------------------------------------------------------------------

OUTPUTS = ("touch", "span", "contained", "repeat", "read", "sum", "err")
OWN = "own"


def raw(eng, form, cols, sym, table, rep, skip=(), n_reads=None, n_rec=None, n_frag=None, n_rep=None):
    """The entry point as the ABI has it; outputs filled with a mark before the call.  table / rep: three arrays (None = NULL), OWN, or ()
    for no annotation.  -> rc, error_index, [touch, span, contained, repeat], read_contained, summary"""
    from raft_amd import engine
    import torch
    lib = engine.load_side_library("frag")
    arrays = lambda t: [None] * 3 if t == OWN or len(t) == 0 else list(t)
    count = lambda t, given: given if given is not None else (-1 if t == OWN else 0 if len(t) == 0 or t[1] is None else t[1].size)
    n_frag, n_rep = count(table, n_frag), count(rep, n_rep)
    rows = max(n_frag, 0) if table != OWN else int(eng.summary.n_fragments)
    table, rep = arrays(table), arrays(rep)
    n_reads = cols[0].size if n_reads is None else n_reads
    n_rec = next(c.size for c in cols[1:] if c is not None) if n_rec is None else n_rec
    read, sm, err = np.full(cols[0].size, -7, np.int32), engine._FragSummary(), C.c_int64(-5)
    sm.n_records = -9
    if form == "device":
        dcols, dtable, drep = on_device(cols), on_device(table), on_device(rep)
        frag = [torch.full((min(rows, 1 << 20),), -7, dtype=torch.int32, device="cuda:0") for _ in range(4)]
        A = lambda t: 0 if t is None else t.data_ptr()
        eng.use_torch_stream()
        fn = lib.raft_hip_frag_overlaps_device
    else:
        keep = lambda xs: [None if a is None else np.ascontiguousarray(a) for a in xs]
        dcols, dtable, drep = keep(cols), keep(table), keep(rep)
        frag = [np.full(min(rows, 1 << 20), -7, np.int32) for _ in range(4)]
        A = lambda a: 0 if a is None else a.ctypes.data
        fn = lib.raft_hip_frag_overlaps_host
    records = engine._Records(n_rec, *[A(c) for c in dcols[1:]])
    t_arg, r_arg = engine._FragTable(n_frag, *[A(a) for a in dtable]), engine._FragTable(n_rep, *[A(a) for a in drep])
    names = dict(zip(OUTPUTS, [C.c_void_p(A(f)) for f in frag] + [C.c_void_p(read.ctypes.data), C.byref(sm), C.byref(err)]))
    outs = [None if k in skip else v for k, v in names.items()]
    rc = fn(eng._ctx, n_reads, C.c_void_p(A(dcols[0])), C.byref(records), int(sym), C.byref(t_arg), C.byref(r_arg), *outs, None)
    if form == "device":
        torch.cuda.synchronize()
        frag = [f.cpu().numpy() for f in frag]
    return rc, err.value, frag, read, sm


def untouched(frag, read, sm):
    return all((f == -7).all() for f in frag) and (read == -7).all() and sm.n_records == -9


@pytest.mark.parametrize("form", ("host", "device"))
def test_an_id_out_of_range_names_the_first_record(eng, form):
    from raft_amd import engine
    cols, table, rep = stream(5000)
    n_reads = cols[0].size
    # several bad records in different workgroups, in either column: the smallest index comes back
    for bad_at in (((1, 4203, n_reads), (4, 1203, -1), (1, 2210, -3)), ((4, 0, n_reads + 7), (1, 4999, -1)), ((1, 4999, n_reads), (4, 4999, -2)),
                   ((4, 3071, 2**31 - 1), (1, 3072, -2**31))):
        bad = [c.copy() for c in cols]
        for col, at, value in bad_at:
            bad[col][at] = value
        for sym in (False, True):
            rc, err, *outs = raw(eng, form, bad, sym, table, rep)
            assert rc == engine.ERR_READ_ID and err == min(at for _, at, _ in bad_at), (bad_at, rc, err)
            assert untouched(*outs), bad_at
    rc, err, *outs = raw(eng, form, cols, False, table, rep)
    assert rc == 0 and err == -1 and not untouched(*outs)


def _violations(table, rep):
    """Each way a table or an annotation can be wrong, by itself."""
    off, fb, fe = table
    count = np.diff(off)
    multi, single = 14, 11                                             # rows [(0, L/3), (L/3, L/3), (L/3, L)] and [(100, L - 100)], behind other reads
    k3, k1 = int(off[multi]), int(off[single])
    assert count[multi] == 3 and fb[k3 + 1] == fe[k3 + 1] == fe[k3] and count[single] == 1 and fb[k1] == 100 and k1 > 0

    def edit(which, k, value):
        out = [off.copy(), fb.copy(), fe.copy()]
        out[which][k] = value
        return tuple(out)

    yield "first offset not 0", edit(0, 0, 1), rep, {}
    yield "offsets step back", edit(0, multi + 1, off[multi] - 1), rep, {}
    yield "last offset short of n_frag", edit(0, len(off) - 1, off[-1] - 1), rep, {}
    yield "last offset beyond the arrays", edit(0, len(off) - 1, off[-1] + 1), rep, {}
    yield "n_frag not the last offset", table, rep, {"n_frag": int(off[-1]) - 1}
    yield "begin descends", edit(1, k3 + 2, fb[k3 + 1] - 1), rep, {}
    yield "end descends", edit(2, k3, fe[k3 + 1] + 1), rep, {}
    yield "begin negative", edit(1, k1, -1), rep, {}
    yield "end before begin", edit(2, k1, fb[k1] - 1), rep, {}
    r_off, r_s, r_e = rep
    with_runs = int(np.flatnonzero(np.diff(r_off) > 0)[2])
    bad = r_off.copy(); bad[with_runs + 1] = r_off[with_runs] - 1
    yield "rep_offset steps back", table, (bad, r_s, r_e), {}
    yield "n_rep not the last rep_offset", table, rep, {"n_rep": r_s.size - 1}
    yield "no frag_offset", (None, fb, fe), rep, {}
    yield "no frag_begin", (off, None, fe), rep, {"n_frag": fe.size}
    yield "no frag_end", (off, fb, None), rep, {}
    yield "arrays but n_frag = -1", table, rep, {"n_frag": -1}
    yield "n_frag = -2", table, rep, {"n_frag": -2}
    yield "no rep_offset", table, (None, r_s, r_e), {}
    yield "no rep_s", table, (r_off, None, r_e), {"n_rep": r_e.size}
    yield "no rep_e", table, (r_off, r_s, None), {}
    yield "arrays but n_rep = -1", table, rep, {"n_rep": -1}
    yield "n_rep = -2", table, rep, {"n_rep": -2}
    yield "n_rec = -1", table, rep, {"n_rec": -1}
    yield "n_reads = -1", table, rep, {"n_reads": -1}


@pytest.mark.parametrize("form", ("host", "device"))
def test_bad_arguments(eng, form):
    from raft_amd import engine
    cols, table, rep = stream(300)
    seen = 0
    for what, bad_table, bad_rep, counts in _violations(table, rep):
        rc, err, *outs = raw(eng, form, cols, False, bad_table, bad_rep, **counts)
        assert rc == engine.ERR_PARAM, (what, rc)
        assert untouched(*outs), what
        seen += 1
    assert seen == 23
    for k in range(1, 7):                                              # a missing column, under either flag
        for sym in (False, True):
            rc, err, *outs = raw(eng, form, cols[:k] + [None] + cols[k + 1:], sym, table, rep)
            assert rc == engine.ERR_PARAM and untouched(*outs), (k, sym)
    for counts in ({"n_rec": 2**30}, {"n_frag": 2**31 - 1}):            # (refused before anything is read)
        rc, err, *outs = raw(eng, form, cols, False, table, rep, **counts)
        assert rc == engine.ERR_TOO_LARGE and untouched(*outs), counts
    rc, err, *outs = raw(eng, form, cols, False, table, rep)           # ... and the context is as good as before
    assert rc == 0 and not untouched(*outs)
    with pytest.raises(ValueError):                                    # (offsets of another number of reads: refused before the library reads them)
        eng.fragment_overlaps(*cols, fragments=(table[0][:-1], table[1], table[2]), repeats=rep)
    descending = (table[0], table[1][::-1].copy(), table[2])
    with pytest.raises(engine.RaftError) as ex:
        eng.fragment_overlaps(*(on_device(cols) if form == "device" else cols), fragments=on_device(descending) if form == "device" else descending,
                              repeats=())
    assert ex.value.code == engine.ERR_PARAM


@pytest.mark.parametrize("form", ("host", "device"))
def test_every_output_null_in_turn(eng, form):
    cols, table, rep = stream(700)
    want = want_fragments(*cols, False, *table, *rep)
    for skip in OUTPUTS + (OUTPUTS,):
        skip = (skip,) if isinstance(skip, str) else skip
        rc, err, frag, read, sm = raw(eng, form, cols, False, table, rep, skip=skip)
        assert rc == 0, skip
        for name, got, exp in zip(OUTPUTS, frag + [read], [want[k] for k in ARRAYS]):
            assert (got == -7).all() if name in skip else np.array_equal(got, exp), (skip, name)
        assert sm.n_records == (-9 if "sum" in skip else 700) and err == (-5 if "err" in skip else -1)
        if "sum" not in skip:
            assert all(getattr(sm, k) == want[k] for k in SUMMARY)


# ---- the goldens, and a context's own pass ------------------------------------------------------------------------------------------------

def _full(eng, s):
    got = eng.fetch()
    got.update(symmetric=s.symmetric, high_cov=s.high_cov, total_coverage=s.total_coverage, total_windows=s.total_windows,
               total_repeat_length=s.total_repeat_length, total_read_length=s.total_read_length)
    return got


@pytest.mark.parametrize("name", GOLDENS)
def test_golden_fixtures_and_the_own_pass(name):
    """The reference's fragment and repeat arrays as explicit arguments, both forms and both flags; then fragments=None, repeats=None after
    a pass of this engine over the golden, in every output width: the same numbers, and the pass's outputs are what they were."""
    from raft_amd import engine
    cols, table, rep = golden_case(name)
    p = RaftParams(**golden_params(name))
    want_pass = oracle_run(p, *cols)
    eng = engine.Engine(p, device=0)
    try:
        want = {sym: check(eng, cols, sym, table, rep, name) for sym in (False, True)}
        seen = classes(want[False], table)
        assert all(v for k, v in seen.items() if k != "untouched"), seen
        for w in WIDTHS:
            eng.set_output_width(w)
            eng.run_host(*cols)
            s = eng.finish()
            fetched = eng.fetch()
            for k, ref in zip(("frag_offset", "frag_begin", "frag_end", "rep_offset", "rep_s", "rep_e"), table + rep):
                assert np.array_equal(fetched[k], ref), (name, w, k)
            for sym in (False, True):
                same_fragments(eng.fragment_overlaps(*cols, symmetric=sym), want[sym], f"{name}, width {w}, own pass, host form")
                same_fragments(eng.fragment_overlaps(*on_device(cols), symmetric=sym), want[sym], f"{name}, width {w}, own pass, device form")
            # one of the two from the pass, the other explicit
            same_fragments(eng.fragment_overlaps(*cols, fragments=table), want[False], f"{name}, width {w}, own annotation")
            same_fragments(eng.fragment_overlaps(*cols, repeats=rep), want[False], f"{name}, width {w}, own table")
            assert_same_result(_full(eng, s), want_pass, f"{name}, width {w}: the pass after the calls")
    finally:
        eng.close()


def test_the_own_pass_needs_a_finished_pass():
    from raft_amd import engine
    from test_read_stats_cases import overlaps_for
    p = RaftParams(est_cov=3, symmetric_mode=1)
    cols = overlaps_for([500, 77, 1200] * 5, 3)
    n_reads = len(cols[0])
    e = np.empty(0, np.int32)
    one_row_each = (np.arange(n_reads + 1, dtype=np.int64), np.zeros(n_reads, np.int32), np.asarray(cols[0], np.int32))
    eng = engine.Engine(p, device=0)

    def state_error():
        for kw in ({}, {"fragments": one_row_each}, {"repeats": (np.zeros(n_reads + 1, np.int64), e, e)}):
            with pytest.raises(engine.RaftError) as ex:
                eng.fragment_overlaps(*cols, **kw)
            assert ex.value.code == engine.ERR_STATE, kw
        got = eng.fragment_overlaps(*cols, fragments=one_row_each, repeats=())                     # explicit arrays: valid in any state
        same_fragments(got, want_fragments(*cols, False, *one_row_each), "explicit arrays")

    state_error()                                                   # no pass at all
    eng.run_host(*cols)
    eng.finish()
    want = oracle_run(p, *cols)
    table, rep = (want["frag_offset"], want["frag_begin"], want["frag_end"]), (want["rep_offset"], want["rep_s"], want["rep_e"])
    same_fragments(eng.fragment_overlaps(*cols), want_fragments(*cols, False, *table, *rep), "after finish")
    with pytest.raises(engine.RaftError) as ex:                      # n_reads is not the pass's
        eng.fragment_overlaps(cols[0][:-1], *cols[1:])
    assert ex.value.code == engine.ERR_PARAM
    eng.run_pipelined(*cols[:4], n_chunks=3)                        # host to host: the context holds no pass afterwards
    state_error()
    bad = [c.copy() for c in cols]
    bad[3][0] = bad[0][bad[1][0]] + 500                             # a record reaching past its read: a data error
    eng.run_host(*bad)
    with pytest.raises(engine.RaftError) as ex:
        eng.finish()
    assert ex.value.code == engine.ERR_COORD
    state_error()
    eng.run_host(*cols)
    eng.finish()
    same_fragments(eng.fragment_overlaps(*cols, symmetric=True), want_fragments(*cols, True, *table, *rep), "after the error")
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
    table = (want_pass["frag_offset"], want_pass["frag_begin"], want_pass["frag_end"])
    rep = (want_pass["rep_offset"], want_pass["rep_s"], want_pass["rep_e"])
    # (query and target are the same read in this set: a mirrored target column gives the sides partners)
    tid = (qid.astype(np.int64) * 7 + 3) % len(rl)
    cols = [rl, qid, a, b, tid.astype(np.int32), np.zeros_like(a), np.minimum(b - a, rl[tid]).astype(np.int32)]
    want = want_fragments(*cols, True, *table, *rep)
    assert (np.diff(table[0]) > 1).any() and want["frags_spanned"] > 0 and want["frags_contained"] > 0
    dev = [torch.from_numpy(x).to("cuda:0") for x in (rl, qid, a, b)]
    eng = engine.Engine(p, device=0)
    for it in range(2):
        eng.run_device(*dev); s = eng.finish()
    assert s.flags & engine.SUM_SPECULATED
    same_fragments(eng.fragment_overlaps(*on_device(cols), symmetric=True), want, "after a speculated pass, device form")
    same_fragments(eng.fragment_overlaps(*cols, symmetric=True), want, "after a speculated pass, host form")
    eng.run_device(*dev); s = eng.finish()
    assert s.flags & engine.SUM_SPECULATED and s.flags & engine.SUM_KEPT_GEOMETRY, s.flags
    assert_same_result(_full(eng, s), want_pass, "the speculated pass behind the call")
    same_fragments(eng.fragment_overlaps(*cols, symmetric=True), want, "after the pass behind the call")
    eng.close()
