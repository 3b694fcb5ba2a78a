"""GPU: raft_hip_repeat_overlaps_device / _host (raft_amd/csrc/ovl_class.hpp, libraft_hip_ovl.so) -- every record classified against the
repeat annotation, the reads' tallies and flags, the summary -- exact against the definitions restated in numpy
(tests/test_repeat_overlaps_cases.py want_classes): at every unit boundary of the record kernel (lane, wave, workgroup, one turn of the
grid-stride loop), on both load paths, in both forms, under symmetric 0 and 1, on the hand-written cases with their literal bytes, on
the golden fixtures with the reference's repeat arrays, against a context's own finished pass in every output width, and in every
state of the context."""
import ctypes as C

import numpy as np
import pytest
from raft_testlib import assert_same_result, oracle_run
from test_repeat_overlaps_cases import (COUNTS, GOLDEN_ANCHORS, HAND, JOIN_COUNTS, SUMMARY, csr, golden_case, golden_params, hand_case, i32, joined_run,
                                        same_classes, stream, want_classes)

from raft_amd.params import RaftParams

pytestmark = pytest.mark.gpu
WIDTHS = (4, 1, 2, 8)          # int32, byte codes, uint16 codes, four-bit steps (RAFT_HIP_COV_DELTA4)


@pytest.fixture(scope="module")
def eng():
    from raft_amd import engine
    e = engine.Engine(RaftParams(est_cov=30), device=0)
    yield e
    e.close()


def on_device(arrays, shift=0):
    """Contiguous CUDA tensors; shift = 1: each begins one element into its allocation, so that no column is 16-byte aligned."""
    import torch
    out = []
    for a in arrays:
        if a is None:
            out.append(None)
            continue
        t = torch.empty(a.size + shift, dtype=torch.from_numpy(a[:0]).dtype, device="cuda:0")
        t[shift:] = torch.from_numpy(np.ascontiguousarray(a))
        out.append(t[shift:])
        assert shift == 0 or out[-1].data_ptr() % 16 != 0 or a.size == 0
    return out


def check(eng, cols, sym, anchor, rep, what, forms=("host", "device"), want=None, shift=0):
    if want is None:
        want = want_classes(*cols, sym, anchor, *rep)
    for form in forms:
        if form == "host":
            got = eng.repeat_overlaps(*cols, min_anchor=anchor, symmetric=sym, repeats=rep)
        else:
            got = eng.repeat_overlaps(*on_device(cols, shift), min_anchor=anchor, symmetric=sym, repeats=on_device(rep))
            assert got["cls"].is_cuda
        same_classes(got, want, f"{what}, {form} form, symmetric {int(sym)}")
        assert eng.last_repeat_overlaps_seconds >= 0.0
        cls = got["cls"].cpu().numpy() if form == "device" else got["cls"]
        # the summary is the sums of the arrays
        assert got["n_records"] == cls.size and got["q_repeat"] == int((cls & 1 != 0).sum()) and got["t_repeat"] == int((cls & 2 != 0).sum())
        assert got["q_touch"] == int((cls & 4 != 0).sum()) and got["t_touch"] == int((cls & 8 != 0).sum()) and got["both_repeat"] == int((cls & 3 == 3).sum())
        assert got["q_contained"] == int((cls & 16 != 0).sum()) and got["t_contained"] == int((cls & 32 != 0).sum())
        assert got["reads_contained"] == int((got["read_flags"] & 1).sum()) and got["reads_repeat_contained"] == int((got["read_flags"] == 1).sum())
    return want


# ---- the record kernel's units ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_rec", COUNTS)
def test_record_counts(eng, n_rec):
    cols, rep = stream(n_rec)
    big = n_rec > 100000           # (one turn of the grid-stride loop: the model once, both forms)
    want = check(eng, cols, False, 300, rep, f"{n_rec} records")
    if n_rec >= 63:
        assert (want["cls"] & 3 != 0).any() and (want["cls"] == 0).any() and (want["cls"] & 48 != 0).any()
    if not big:
        check(eng, cols, True, 300, rep, f"{n_rec} records")


@pytest.mark.parametrize("n_rec", (1, 5, 257, 1025))
def test_columns_offset_by_one_element(eng, n_rec):
    """No column is 16-byte aligned: the 4-byte load path, the same bytes."""
    cols, rep = stream(n_rec, seed=9)
    for sym in (False, True):
        check(eng, cols, sym, 300, rep, f"{n_rec} records, shifted", forms=("device",), shift=1)


@pytest.mark.parametrize("n_rec", (3, 64, 1025))
def test_without_target_columns(eng, n_rec):
    cols, rep = stream(n_rec, seed=3)
    cols = cols[:5] + [None, None]
    want = check(eng, cols, True, 300, rep, f"{n_rec} records, no ts / te")
    assert (want["cls"] & (2 | 8 | 32) == 0).all()
    from raft_amd import engine
    with pytest.raises(ValueError):
        eng.repeat_overlaps(*cols, min_anchor=300, symmetric=False, repeats=rep)
    rc, *_ = raw(eng, "host", cols, False, 300, rep)                     # (the ABI: a missing column)
    assert rc == engine.ERR_PARAM


@pytest.mark.parametrize("flagged", (True, False), ids=("all_flagged", "none_flagged"))
@pytest.mark.parametrize("n_rec", JOIN_COUNTS)
def test_one_id_across_lanes_waves_and_workgroups(eng, n_rec, flagged):
    cols, rep = joined_run(n_rec, flagged)
    for sym in (False, True):
        want = check(eng, cols, sym, 100000, rep, f"one id over {n_rec} records")
        q = 0 if flagged else 2
        assert want["read_touch"][q] == want["read_repeat"][q] == (n_rec if flagged else 0)
        assert want["read_touch"][q + 1] == (n_rec if flagged and not sym else 0)


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_written_cases(eng, name):
    cols, sym, anchor, rep, exp = hand_case(name)
    want = check(eng, cols, sym, anchor, rep, name)
    for k, v in exp.items():
        assert np.array_equal(want[k], v), (name, k)
    if name == "symmetric_counts_query_sides":
        check(eng, cols[:5] + [None, None], True, anchor, rep, name + ", no ts / te")


def test_forty_runs_and_every_min_anchor(eng):
    """A read of 40 runs: sides that bridge 1, 2, ..., 40 of them, under min_anchor from 1 up to INT32_MAX."""
    L = 41 * 300
    runs = [[(k * 300 + 10, k * 300 + 160) for k in range(40)], []]
    rep = csr(runs)
    n = 40
    cols = [i32(L, L + 5), np.zeros(n, np.int32), np.full(n, 10, np.int32), i32(*[k * 300 + 160 for k in range(n)]), np.ones(n, np.int32),
            np.zeros(n, np.int32), np.full(n, L + 5, np.int32)]
    for anchor in (1, 150, 151, 5851, 2**31 - 1):
        want = check(eng, cols, False, anchor, rep, f"40 runs, min_anchor {anchor}")
        assert int((want["cls"] & 1).sum()) == {1: 1, 150: 1, 151: 2, 5851: 40, 2**31 - 1: 40}[anchor]


def test_no_reads_and_no_records(eng):
    e = np.empty(0, np.int32)
    check(eng, [e] * 7, False, 1000, (np.zeros(1, np.int64), e, e), "no reads")
    cols, rep = stream(5)
    check(eng, [cols[0]] + [e] * 6, False, 1000, rep, "no records")
    check(eng, [cols[0]] + [e] * 6, True, 1000, rep, "no records")


# ---- the ABI: errors, NULL outputs ----------------------------------------------------------------------------------------------------------

def raw(eng, form, cols, sym, anchor, rep, n_rep=None, skip=()):
    """The entry point as the ABI has it; outputs filled with a mark before the call.  -> rc, error_index, cls, touch, repeat, flags, summary"""
    from raft_amd import engine
    import torch
    lib = engine.load_side_library("ovl")
    n_reads, n_rec = cols[0].size, cols[1].size
    touch, repeat, flags = np.full(n_reads, -7, np.int32), np.full(n_reads, -7, np.int32), np.full(n_reads, 77, np.uint8)
    sm, err = engine._OvlSummary(), C.c_int64(-5)
    sm.n_records = -9
    if n_rep is None:
        n_rep = -1 if rep is None else (rep[1].size if rep[1] is not None else 0)
    rep = [None] * 3 if rep is None else rep
    if form == "device":
        dcols, drep = on_device(cols), on_device(rep)
        cls = torch.full((n_rec,), 77, dtype=torch.uint8, device="cuda:0")
        P = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
        eng.use_torch_stream()
        fn = lib.raft_hip_repeat_overlaps_device
    else:
        dcols, drep = [None if a is None else np.ascontiguousarray(a) for a in cols], [None if a is None else np.ascontiguousarray(a) for a in rep]
        cls = np.full(n_rec, 77, np.uint8)
        P = lambda a: C.c_void_p(0 if a is None else a.ctypes.data)
        fn = lib.raft_hip_repeat_overlaps_host
    H = lambda a: C.c_void_p(a.ctypes.data)
    outs = [None if "cls" in skip else P(cls), None if "touch" in skip else H(touch), None if "repeat" in skip else H(repeat),
            None if "flags" in skip else H(flags), None if "sum" in skip else C.byref(sm), None if "err" in skip else C.byref(err)]
    rc = fn(eng._ctx, n_reads, P(dcols[0]), n_rec, *[P(c) for c in dcols[1:]], int(sym), anchor, n_rep, *[P(a) for a in drep], *outs, None)
    if form == "device":
        torch.cuda.synchronize()
        cls = cls.cpu().numpy()
    return rc, err.value, cls, touch, repeat, flags, sm


def untouched(cls, touch, repeat, flags, sm):
    return (cls == 77).all() and (touch == -7).all() and (repeat == -7).all() and (flags == 77).all() and sm.n_records == -9


@pytest.mark.parametrize("form", ("host", "device"))
def test_an_id_out_of_range_in_each_column(eng, form):
    from raft_amd import engine
    cols, rep = stream(1500)
    n_reads = cols[0].size
    for col, at, value in ((1, 1203, n_reads), (4, 1203, -1), (1, 0, -3), (4, 1499, n_reads + 7)):
        bad = [c.copy() for c in cols]
        bad[col][at] = value
        if col == 1:
            bad[4][at + 1 if at + 1 < 1500 else at] = n_reads          # (a later record, or the same one's target: the first record wins, the query first)
        rc, err, *outs = raw(eng, form, bad, False, 300, rep)
        assert rc == engine.ERR_READ_ID and err == at, (col, at, rc, err)
        assert untouched(*outs), (col, at)
    rc, err, *outs = raw(eng, form, cols, False, 300, rep)
    assert rc == 0 and err == -1 and not untouched(*outs)


@pytest.mark.parametrize("form", ("host", "device"))
def test_bad_arguments(eng, form):
    from raft_amd import engine
    cols, rep = stream(300)
    off, s, e = rep
    r = int(np.flatnonzero((np.diff(off) == 0) & (off[:-1] > 0))[3])              # a read without runs, behind some with
    for what, bad_rep, n_rep in (("descending", (np.r_[off[:r + 1], off[r] - 1, off[r + 2:]], s, e), None),
                                 ("first not 0", (np.r_[1, off[1:]], s, e), None),
                                 ("wrong total", (off, s, e), s.size - 1),
                                 ("total beyond the arrays", (np.r_[off[:-1], off[-1] + 1], s, e), None),
                                 ("no offsets", (None, s, e), None), ("no starts", (off, None, e), s.size), ("no ends", (off, s, None), None),
                                 ("arrays but n_rep = -1", (off, s, e), -1), ("n_rep = -2", (off, s, e), -2)):
        rc, err, *outs = raw(eng, form, cols, False, 300, bad_rep, n_rep=n_rep)
        assert rc == engine.ERR_PARAM, (what, rc)
        assert untouched(*outs), what
    for anchor in (0, -1):
        rc, err, *outs = raw(eng, form, cols, False, anchor, rep)
        assert rc == engine.ERR_PARAM and untouched(*outs), anchor
    rc, err, *outs = raw(eng, form, cols, False, 300, rep)                       # ... and the context is as good as before
    assert rc == 0
    with pytest.raises(engine.RaftError) as ex:
        eng.repeat_overlaps(*cols, min_anchor=0, repeats=rep)
    assert ex.value.code == engine.ERR_PARAM


@pytest.mark.parametrize("form", ("host", "device"))
def test_every_output_null_in_turn(eng, form):
    cols, rep = stream(700)
    want = want_classes(*cols, False, 300, *rep)
    for skip in ("cls", "touch", "repeat", "flags", "sum", "err", ("cls", "touch", "repeat", "flags", "sum", "err")):
        skip = (skip,) if isinstance(skip, str) else skip
        rc, err, cls, touch, repeat, flags, sm = raw(eng, form, cols, False, 300, rep, skip=skip)
        assert rc == 0, skip
        for name, got, exp in (("cls", cls, want["cls"]), ("touch", touch, want["read_touch"]), ("repeat", repeat, want["read_repeat"]),
                               ("flags", flags, want["read_flags"])):
            assert (np.unique(got).tolist() in ([77], [-7])) if name in skip else np.array_equal(got, exp), (skip, name)
        assert sm.n_records == (-9 if "sum" in skip else 700) and err == (-5 if "err" in skip else -1)
        if "sum" not in skip:
            assert all(getattr(sm, k) == want[k] for k in SUMMARY)


# ---- the goldens, and a context's own pass ------------------------------------------------------------------------------------------------

def _full(eng, s):
    got = eng.fetch()
    got.update(symmetric=s.symmetric, high_cov=s.high_cov, total_coverage=s.total_coverage, total_windows=s.total_windows,
               total_repeat_length=s.total_repeat_length, total_read_length=s.total_read_length)
    return got


@pytest.mark.parametrize("name", sorted(GOLDEN_ANCHORS))
def test_golden_fixtures_and_the_own_pass(name):
    """The reference's repeat arrays as explicit annotation, both forms and both flags; then repeats=None after a pass of this engine over
    the golden -- in every output width, after a bucketed pass and after a second run_device over the same tensors -- equals the call
    with the arrays fetched from that pass and the model on the golden's arrays; the pass's outputs are what they were."""
    from raft_amd import engine
    cols, rep = golden_case(name)
    anchor = GOLDEN_ANCHORS[name]
    p = RaftParams(**golden_params(name))
    want_pass = oracle_run(p, *cols)
    eng = engine.Engine(p, device=0)
    try:
        want = {sym: check(eng, cols, sym, anchor, rep, name) for sym in (False, True)}
        assert (want[False]["cls"] & 3 != 0).any() and (want[False]["cls"] & 12 != 0).any()

        def own(what, s):
            fetched = eng.fetch()
            assert np.array_equal(fetched["rep_offset"], rep[0]) and np.array_equal(fetched["rep_s"], rep[1]) and np.array_equal(fetched["rep_e"], rep[2])
            for sym in (False, True):
                same_classes(eng.repeat_overlaps(*cols, min_anchor=anchor, symmetric=sym), want[sym], f"{name}, {what}, own pass, host form")
                got = eng.repeat_overlaps(*on_device(cols), min_anchor=anchor, symmetric=sym)
                same_classes(got, want[sym], f"{name}, {what}, own pass, device form")
                explicit = eng.repeat_overlaps(*cols, min_anchor=anchor, symmetric=sym, repeats=(fetched["rep_offset"], fetched["rep_s"], fetched["rep_e"]))
                same_classes(explicit, want[sym], f"{name}, {what}, fetched arrays")
            assert_same_result(_full(eng, s), want_pass, f"{name}, {what}: the pass after the call")

        for w in WIDTHS:
            eng.set_output_width(w)
            eng.run_host(*cols)
            own(f"width {w}", eng.finish())
        eng.set_output_width(4)
        eng.set_tuning(0, True)
        eng.run_host(*cols)
        s = eng.finish()
        assert s.interval_path == 1
        own("bucketed", s)
        eng.set_tuning(0, False)
        dev = on_device(cols)
        for it in range(2):
            eng.run_device(*dev)
            own(f"run_device {it}", eng.finish())
    finally:
        eng.close()


def test_the_own_pass_needs_a_finished_pass():
    from raft_amd import engine
    from test_read_stats_cases import overlaps_for
    p = RaftParams(est_cov=3, symmetric_mode=1)
    cols = overlaps_for([500, 77, 1200] * 5, 3)
    explicit = (np.zeros(16, np.int64), np.empty(0, np.int32), np.empty(0, np.int32))
    eng = engine.Engine(p, device=0)

    def state_error():
        with pytest.raises(engine.RaftError) as e:
            eng.repeat_overlaps(*cols, min_anchor=10)
        assert e.value.code == engine.ERR_STATE
        assert eng.repeat_overlaps(*cols, min_anchor=10, repeats=explicit)["q_touch"] == 0          # explicit arrays: valid in any state

    state_error()                                                   # no pass at all
    eng.run_host(*cols)
    eng.finish()
    want = oracle_run(p, *cols)
    rep = (want["rep_offset"], want["rep_s"], want["rep_e"])
    same_classes(eng.repeat_overlaps(*cols, min_anchor=10), want_classes(*cols, False, 10, *rep), "after finish")
    with pytest.raises(engine.RaftError) as e:                       # n_reads is not the pass's
        eng.repeat_overlaps(cols[0][:-1], *cols[1:], min_anchor=10)
    assert e.value.code == engine.ERR_PARAM
    eng.run_pipelined(*cols[:4], n_chunks=3)                        # host to host: the context holds no pass afterwards
    state_error()
    bad = [c.copy() for c in cols]
    bad[3][0] = bad[0][bad[1][0]] + 500                             # a record reaching past its read: a data error
    eng.run_host(*bad)
    with pytest.raises(engine.RaftError) as e:
        eng.finish()
    assert e.value.code == engine.ERR_COORD
    state_error()
    eng.run_host(*cols)
    eng.finish()
    same_classes(eng.repeat_overlaps(*cols, min_anchor=10, symmetric=True), want_classes(*cols, True, 10, *rep), "after the error")
    eng.close()


def test_the_call_hands_out_no_geometry():
    """After a speculated pass the own-pass call answers as after any other, and the pass behind it is speculated on kept geometry."""
    import torch
    from raft_amd import engine
    from test_gpu_speculate import _set
    p = RaftParams(est_cov=4, repeat_length=2000, interval_length=2000, symmetric_mode=1)       # (1328 repeats, up to four on a read)
    rl, (qid, a, b) = _set(31)
    cols = [rl, qid, a, b, qid, a, b]
    want_pass = oracle_run(p, *cols); want_pass["symmetric"] = 1      # (asserted by the parameters, not detected)
    rep = (want_pass["rep_offset"], want_pass["rep_s"], want_pass["rep_e"])
    want = want_classes(*cols, True, 2000, *rep)
    assert (np.diff(rep[0]) > 1).any() and (want["cls"] & 1 != 0).any() and (want["cls"] & 5 == 4).any() and (want["cls"] == 0).any()
    dev = [torch.from_numpy(x).to("cuda:0") for x in (rl, qid, a, b)]
    eng = engine.Engine(p, device=0)
    for it in range(2):
        eng.run_device(*dev); s = eng.finish()
    assert s.flags & engine.SUM_SPECULATED
    same_classes(eng.repeat_overlaps(*dev, dev[1], dev[2], dev[3], min_anchor=2000, symmetric=True), want, "after a speculated pass, device form")
    same_classes(eng.repeat_overlaps(*cols, min_anchor=2000, symmetric=True), want, "after a speculated pass, host form")
    eng.run_device(*dev); s = eng.finish()
    assert s.flags & engine.SUM_SPECULATED and s.flags & engine.SUM_KEPT_GEOMETRY, s.flags
    assert_same_result(_full(eng, s), want_pass, "the speculated pass behind the call")
    same_classes(eng.repeat_overlaps(*cols, min_anchor=2000, symmetric=True), want, "after the pass behind the call")
    eng.close()
