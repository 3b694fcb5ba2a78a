"""GPU: raft_hip_lift_overlaps_device / _host (raft_amd/csrc/lift.hpp, libraft_hip_lift.so) -- every record cut at the fragment bounds of
both of its reads and shifted into fragment coordinates -- exact against the brute-force oracle of tests/lift_testlib.py on every
column, on the order and on the summary: at the lane, wave and tile boundaries of the record kernels, on tables that mix reads of 0 to
40 rows whose rows overlap by 0, 10 and 500 bases, on the fast path alone, with one lane writing 1600 outputs, on tiles that are all
cut and all empty, on both load paths, in both forms, under both strands and three values of min_len, with every capacity around
n_out, every refusal of the header, against a context's own finished pass and in every state of the context."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from lift_testlib import COLUMNS, SUMMARY, as_multiset, identity_table, lift, make_stream, make_table, mirror
from raft_testlib import ROOT, assert_same_result, oracle_run

from raft_amd.params import RaftParams

pytestmark = pytest.mark.gpu
FORMS = ("host", "device")


def _constant(header, name):
    text = open(os.path.join(ROOT, "raft_amd", "csrc", header)).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


T = _constant("record_stream.hpp", "kStreamThreads") * _constant("record_stream.hpp", "kStreamLaneRecords")
MAX_BLOCKS = _constant("record_stream.hpp", "kStreamMaxBlocks")
SIZES = [0, 1, 3, 4, 5, 255, 256, 257, T - 1, T, T + 1, 2 * T + 3]


def test_the_constants_are_the_expected_ones():
    text = open(os.path.join(ROOT, "raft_amd", "csrc", "lift.hpp")).read()
    assert "constexpr int kLiftTile = kStreamThreads * kStreamLaneRecords;" in text and T == 1024 and MAX_BLOCKS == 2048


@pytest.fixture(scope="module")
def eng():
    from raft_amd import engine
    e = engine.Engine(RaftParams(est_cov=3), device=0)
    yield e
    e.close()


def on_device(arrays, shift=0):
    """Contiguous CUDA tensors; shift = 1: each begins one element into its allocation, so that no column is on a 16-byte line."""
    import torch
    out = []
    for a in arrays:
        t = torch.empty(a.size + shift, dtype=torch.from_numpy(a[:0]).dtype, device="cuda:0")
        t[shift:] = torch.from_numpy(np.ascontiguousarray(a))
        out.append(t[shift:])
        assert shift == 0 or a.size == 0 or out[-1].data_ptr() % 16 != 0
    return out


def same(got, want, what):
    for k in SUMMARY:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in COLUMNS:
        g = got[k].cpu().numpy() if hasattr(got[k], "is_cuda") else np.asarray(got[k])
        w = want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, f"{what}: {k} differs at {bad.size} of {w.size} outputs, first at {bad[0]}: got {g[bad[0]]} want {w[bad[0]]}"


def check(eng, cols, strand, table, min_len, what, forms=FORMS, want=None, shift=0):
    if want is None:
        want = lift(*table, cols, strand, min_len)
    for form in forms:
        if form == "host":
            got = eng.lift_overlaps(*cols, strand, fragments=table, min_len=min_len)
        else:
            got = eng.lift_overlaps(*on_device(cols, shift), *on_device([strand], shift), fragments=on_device(table), min_len=min_len)
            assert all(got[k].is_cuda for k in COLUMNS)
        same(got, want, f"{what}, {form} form, min_len {min_len}")
        assert got["kernel_seconds"] >= 0.0 and eng.last_lift_overlaps_seconds == got["kernel_seconds"]
    return want


@pytest.fixture(scope="module")
def mixed():
    """The table of most tests: 60 reads of 0, 1, 2, 3 and 40 rows whose rows overlap by 0, 10 and 500 bases."""
    rng = np.random.default_rng(11)
    read_len, off, fb, fe = make_table(rng, 60)
    rows = np.diff(off)
    assert set(rows.tolist()) == {0, 1, 2, 3, 40}
    return read_len, (off, fb, fe)


# ---- the record kernels' units --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_rec", SIZES)
def test_record_counts(eng, mixed, n_rec):
    read_len, table = mixed
    cols, strand = make_stream(np.random.default_rng(100 + n_rec), read_len, n_rec)
    want = check(eng, cols, strand, table, 1, f"{n_rec} records")
    if n_rec >= 255:
        assert want["records_cut"] > 0 and want["records_none"] > 0 and want["most_per_record"] > 4 and 0 < want["n_out"] != n_rec
        assert set(want["rev"].tolist()) == {0, 1}


@pytest.mark.parametrize("n_rec", (5, 257, T + 1, 2 * T + 3))
def test_columns_offset_by_one_element(eng, mixed, n_rec):
    """No column begins on a 16-byte line, the strand bytes on no 4-byte one: the element-access path, the same outputs."""
    read_len, table = mixed
    cols, strand = make_stream(np.random.default_rng(7 + n_rec), read_len, n_rec)
    check(eng, cols, strand, table, 1, f"{n_rec} records, shifted", forms=("device",), shift=1)


@pytest.mark.parametrize("rev", (0, 1))
def test_the_fast_path_alone(eng, rev):
    """One whole-read row per read: the output equals the input (but for the records of a read with itself)."""
    rng = np.random.default_rng(5 + rev)
    read_len = rng.integers(100, 30000, 50).astype(np.int32)
    n = 2 * T + 3
    qid = rng.integers(0, 50, n).astype(np.int32)
    tid = ((qid + 1 + rng.integers(0, 49, n)) % 50).astype(np.int32)
    qs = (rng.random(n) * (read_len[qid] - 1)).astype(np.int32); qe = (qs + 1 + rng.random(n) * (read_len[qid] - qs - 1)).astype(np.int32)
    ts = (rng.random(n) * (read_len[tid] - 1)).astype(np.int32); te = (ts + 1 + rng.random(n) * (read_len[tid] - ts - 1)).astype(np.int32)
    cols, strand = [qid, qs, qe, tid, ts, te], np.full(n, rev, np.uint8)
    want = dict(zip(COLUMNS, cols + [strand, np.arange(n, dtype=np.int32)]))
    want.update(n_records=n, n_out=n, records_none=0, records_cut=0, pairs_dropped=0, most_per_record=1)
    check(eng, cols, strand, identity_table(read_len), 1, "identity table", want=want)


def test_two_reads_of_forty_rows(eng, mixed):
    """One record over all 40 x 40 row pairs, among others: the pair loop, and the ranks in a tile when one lane writes many outputs."""
    read_len, (off, fb, fe) = mixed
    a, b = np.flatnonzero(np.diff(off) == 40)[:2]
    cols, strand = make_stream(np.random.default_rng(3), read_len, T + 7)
    for at, rev in ((0, 0), (517, 1), (T - 1, 0), (T + 6, 1)):
        for k, v in enumerate((a, 0, read_len[a], b, 0, read_len[b])):
            cols[k][at] = v
        strand[at] = rev
    want = check(eng, cols, strand, (off, fb, fe), 1, "40 x 40")
    # (every row of a meets the image of two or three rows of b: far fewer than 1600 pairs survive, all 1600 are looked at)
    assert want["most_per_record"] >= 40 and want["pairs_dropped"] >= 4 * (1600 - want["most_per_record"])
    check(eng, cols, strand, (off, fb, fe), 501, "40 x 40")


def test_a_tile_in_which_every_record_is_cut_and_one_in_which_none_lifts(eng, mixed):
    read_len, (off, fb, fe) = mixed
    rows = np.diff(off)
    three, empty = np.flatnonzero(rows == 3)[:2], np.flatnonzero(rows == 0)[:2]
    n = 3 * T
    qid = np.empty(n, np.int32); tid = np.empty(n, np.int32)
    qid[:T], tid[:T] = three[0], three[1]                   # tile 0: whole reads of three rows each: every record is cut
    qid[T:2 * T], tid[T:2 * T] = empty[0], three[1]         # tile 1: a read without rows: nothing lifts
    qid[2 * T:], tid[2 * T:] = three[1], three[0]
    qs, ts = np.zeros(n, np.int32), np.zeros(n, np.int32)
    qe, te = read_len[qid].astype(np.int32), read_len[tid].astype(np.int32)
    strand = (np.arange(n) % 2).astype(np.uint8)
    want = check(eng, [qid, qs, qe, tid, ts, te], strand, (off, fb, fe), 1, "all cut, none, all cut")
    per = np.bincount(want["src"], minlength=n)
    assert per[:T].min() > 1 and per[T:2 * T].max() == 0 and per[2 * T:].min() > 1
    assert want["records_cut"] == 2 * T and want["records_none"] == T


def test_more_tiles_than_the_capped_grid(eng):
    """MAX_BLOCKS * T + 1 records: the grid-stride loop of both kernels; the identity table, so that the oracle is the input itself."""
    import torch
    n = MAX_BLOCKS * T + 1
    n_reads = 1000
    read_len = np.full(n_reads, 5000, np.int32)
    i = np.arange(n, dtype=np.int64)
    qid = (i % n_reads).astype(np.int32); tid = ((i + 1 + i // n_reads % (n_reads - 1)) % n_reads).astype(np.int32)
    qs = (i % 997).astype(np.int32); qe = (qs + 1 + i % 3001).astype(np.int32)
    ts = (i % 1009).astype(np.int32); te = (ts + 1 + i % 2999).astype(np.int32)
    strand = (i % 2).astype(np.uint8)
    assert (qid != tid).all() and qe.max() <= 5000 and te.max() <= 5000
    cols = [qid, qs, qe, tid, ts, te]
    got = eng.lift_overlaps(*on_device(cols), *on_device([strand]), fragments=on_device(identity_table(read_len)))
    assert got["n_out"] == n and got["records_none"] == 0 and got["records_cut"] == 0 and got["most_per_record"] == 1
    for k, w in zip(COLUMNS, cols + [strand, np.arange(n, dtype=np.int32)]):
        assert torch.equal(got[k].cpu(), torch.from_numpy(w)), k


# ---- the rule ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("min_len", (1, 2, 501))
@pytest.mark.parametrize("rev", (0, 1))
def test_min_len_and_strand(eng, mixed, min_len, rev):
    """... with a pair of exactly min_len and one of min_len - 1, on either side"""
    read_len, (off, fb, fe) = mixed
    cols, strand = make_stream(np.random.default_rng(40 + min_len + rev), read_len, 600, rev=rev)
    rows = np.diff(off)
    one, two = int(np.flatnonzero(rows == 1)[0]), int(np.flatnonzero(rows == 2)[0])
    L = min_len
    # A side (the smaller id's) exactly L and L - 1 inside one row each; then the same on the B side, the A side longer
    lo, hi = min(one, two), max(one, two)
    klo, khi = int(off[lo]), int(off[hi])
    edge = []
    for la, lb in ((L, L + 5), (L - 1, L + 5), (L + 5, L), (L + 5, L - 1), (L, L), (L - 1, L - 1)):
        if la > 0 and lb > 0:
            edge.append((lo, fb[klo] + 3, fb[klo] + 3 + la, hi, fb[khi] + 2, fb[khi] + 2 + lb))
            edge.append((hi, fb[khi] + 2, fb[khi] + 2 + lb, lo, fb[klo] + 3, fb[klo] + 3 + la))
    for at, rec in enumerate(edge):
        for k in range(6):
            cols[k][at * 7] = rec[k]
    want = check(eng, cols, strand, (off, fb, fe), min_len, f"rev {rev}")
    per = np.bincount(want["src"], minlength=600)
    kept = [bool(per[at * 7]) for at in range(len(edge))]
    expect = [la >= L and lb >= L for la, lb in ((L, L + 5), (L - 1, L + 5), (L + 5, L), (L + 5, L - 1), (L, L), (L - 1, L - 1)) if la > 0 and lb > 0 for _ in (0, 1)]
    assert kept == expect and want["pairs_dropped"] >= expect.count(False)


def test_the_mirror_property_on_a_symmetric_stream(eng, mixed):
    read_len, table = mixed
    cols, strand = make_stream(np.random.default_rng(77), read_len, 700)
    mcols, mstrand = mirror(cols, strand)
    both = [np.concatenate([a, b]) for a, b in zip(cols, mcols)]
    bstrand = np.concatenate([strand, mstrand])
    for min_len in (1, 501):
        got = eng.lift_overlaps(*both, bstrand, fragments=table, min_len=min_len)
        first = {k: got[k][got["src"] < 700] for k in COLUMNS}
        second = {k: got[k][got["src"] >= 700] for k in COLUMNS}
        assert first["src"].size > 100 and as_multiset(first) == as_multiset(second, mirrored=True)
        same(got, lift(*table, both, bstrand, min_len), "symmetric stream")


# ---- the ABI: capacities, errors, NULL outputs ------------------------------------------------------------------------------------------

OWN = "own"
NAMES = COLUMNS + ("sum", "err")


def raw(eng, form, cols, strand, table, min_len=1, out_cap=None, skip=(), n_reads=None, n_rec=None, n_frag=None, room=None):
    """The entry point as the ABI has it; outputs filled with a mark before the call.  table: three arrays (None = NULL) or OWN.
    -> rc, error_index, the eight columns (of `room` elements), summary"""
    from raft_amd import engine
    import torch
    lib = engine.load_side_library("lift")
    tab = [None] * 3 if table == OWN else list(table)
    if n_frag is None:
        n_frag = -1 if table == OWN else (0 if tab[1] is None else tab[1].size)
    if n_reads is None:
        n_reads = int(eng.summary.n_reads) if table == OWN else (tab[0].size - 1 if tab[0] is not None else 0)
    if n_rec is None:
        n_rec = next(c.size for c in cols if c is not None)
    room = (out_cap if out_cap is not None else 0) if room is None else room
    out_cap = room if out_cap is None else out_cap
    sm, err = engine._LiftSummary(), C.c_int64(-5)
    sm.n_records = -9
    dtypes = [np.uint8 if k == "rev" else np.int32 for k in COLUMNS]
    if form == "device":
        put = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
        dcols, dstrand, dtab = [put(c) for c in cols], put(strand), [put(a) for a in tab]
        outs = [torch.full((room,), 249, dtype=torch.from_numpy(np.empty(0, d)).dtype, device="cuda:0") for d in dtypes]
        A = lambda t: 0 if t is None or t.numel() == 0 else t.data_ptr()
        eng.use_torch_stream()
        fn = lib.raft_hip_lift_overlaps_device
    else:
        keep = lambda a: None if a is None else np.ascontiguousarray(a)
        dcols, dstrand, dtab = [keep(c) for c in cols], keep(strand), [keep(a) for a in tab]
        outs = [np.full(room, 249, d) for d in dtypes]
        A = lambda a: 0 if a is None or a.size == 0 else a.ctypes.data
        fn = lib.raft_hip_lift_overlaps_host
    records = engine._Records(n_rec, *[A(c) for c in dcols])
    t_arg = engine._FragTable(n_frag, *[A(a) for a in dtab])
    names = dict(zip(NAMES, [C.c_void_p(A(o)) for o in outs] + [C.byref(sm), C.byref(err)]))
    args = [None if k in skip else v for k, v in names.items()]
    rc = fn(eng._ctx, n_reads, C.byref(records), C.c_void_p(A(dstrand)), C.byref(t_arg), min_len, out_cap, *args, None)
    if form == "device":
        torch.cuda.synchronize()
        outs = [o.cpu().numpy() for o in outs]
    return rc, err.value, outs, sm


def untouched(outs, sm=None):
    return all((o == 249).all() for o in outs) and (sm is None or sm.n_records == -9)


@pytest.mark.parametrize("form", FORMS)
def test_capacities_around_n_out(eng, mixed, form):
    from raft_amd import engine
    read_len, table = mixed
    cols, strand = make_stream(np.random.default_rng(8), read_len, 900)
    want = lift(*table, cols, strand)
    n_out = want["n_out"]
    assert n_out > 900
    # the size query: every output NULL, whatever the capacity
    for cap in (0, n_out - 1, n_out):
        rc, err, outs, sm = raw(eng, form, cols, strand, table, out_cap=cap, skip=COLUMNS, room=4)
        assert rc == 0 and err == -1 and untouched(outs) and all(getattr(sm, k) == want[k] for k in SUMMARY)
    # one short: nothing is written, the summary says what is needed
    rc, err, outs, sm = raw(eng, form, cols, strand, table, out_cap=n_out - 1, room=n_out + 3)
    assert rc == engine.ERR_TOO_LARGE and untouched(outs) and sm.n_out == n_out and err == -1
    rc, err, outs, sm = raw(eng, form, cols, strand, table, out_cap=0, room=n_out + 3, skip=COLUMNS[1:])
    assert rc == engine.ERR_TOO_LARGE and untouched(outs) and sm.n_out == n_out
    # exactly enough, and more than enough: nothing behind n_out is written
    for cap in (n_out, n_out + 3):
        rc, err, outs, sm = raw(eng, form, cols, strand, table, out_cap=cap, room=n_out + 3)
        assert rc == 0 and err == -1
        for k, o in zip(COLUMNS, outs):
            assert np.array_equal(o[:n_out], want[k]) and (o[n_out:] == 249).all(), k


@pytest.mark.parametrize("form", FORMS)
def test_every_output_null_in_turn(eng, mixed, form):
    read_len, table = mixed
    cols, strand = make_stream(np.random.default_rng(9), read_len, 700)
    want = lift(*table, cols, strand)
    n_out = want["n_out"]
    for skip in NAMES:
        rc, err, outs, sm = raw(eng, form, cols, strand, table, out_cap=n_out, skip=(skip,))
        assert rc == 0, skip
        for k, o in zip(COLUMNS, outs):
            assert (o == 249).all() if k == skip else np.array_equal(o, want[k]), (skip, k)
        assert sm.n_records == (-9 if skip == "sum" else 700) and err == (-5 if skip == "err" else -1)


@pytest.mark.parametrize("form", FORMS)
def test_an_id_out_of_range_names_the_first_record(eng, mixed, form):
    from raft_amd import engine
    read_len, table = mixed
    cols, strand = make_stream(np.random.default_rng(10), read_len, 5000)
    n_reads = read_len.size
    n_out = lift(*table, cols, strand)["n_out"]
    for bad_at in (((0, 4203, n_reads), (3, 1203, -1), (0, 2210, -3)), ((3, 0, n_reads + 7), (0, 4999, -1)), ((0, 4999, n_reads), (3, 4999, -2)),
                   ((3, 3071, 2**31 - 1), (0, 3072, -2**31))):
        bad = [c.copy() for c in cols]
        for col, at, value in bad_at:
            bad[col][at] = value
        rc, err, outs, sm = raw(eng, form, bad, strand, table, out_cap=n_out + 5000)
        assert rc == engine.ERR_READ_ID and err == min(at for _, at, _ in bad_at), (bad_at, rc, err)
        assert untouched(outs, sm), bad_at
    rc, err, outs, sm = raw(eng, form, cols, strand, table, out_cap=n_out)
    assert rc == 0 and err == -1 and not untouched(outs, sm)


def _broken_tables(table):
    off, fb, fe = table
    rows = np.diff(off)
    multi, single = int(np.flatnonzero(rows == 3)[0]), int(np.flatnonzero(rows == 1)[0])
    k3, k1 = int(off[multi]), int(off[single])

    def edit(which, k, value):
        out = [off.copy(), fb.copy(), fe.copy()]
        out[which][k] = value
        return tuple(out)

    yield "first offset not 0", edit(0, 0, 1), {}
    yield "offsets step back", edit(0, multi + 1, off[multi] - 1), {}
    yield "last offset short of n_frag", edit(0, len(off) - 1, off[-1] - 1), {}
    yield "last offset beyond the arrays", edit(0, len(off) - 1, off[-1] + 1), {}
    yield "n_frag not the last offset", table, {"n_frag": int(off[-1]) - 1}
    yield "begin descends", edit(1, k3 + 2, fb[k3 + 1] - 1), {}
    yield "end descends", edit(2, k3, fe[k3 + 1] + 1), {}
    yield "begin negative", edit(1, k1, -1), {}
    yield "end before begin", edit(2, k1, fb[k1] - 1), {}


@pytest.mark.parametrize("form", FORMS)
def test_a_broken_table(eng, mixed, form):
    from raft_amd import engine
    read_len, table = mixed
    cols, strand = make_stream(np.random.default_rng(12), read_len, 300)
    seen = 0
    for what, bad, counts in _broken_tables(table):
        rc, err, outs, sm = raw(eng, form, cols, strand, bad, out_cap=100000, room=64, **counts)
        assert rc == engine.ERR_PARAM and untouched(outs, sm), (what, rc)
        seen += 1
    assert seen == 9
    with pytest.raises(engine.RaftError) as ex:
        eng.lift_overlaps(*cols, strand, fragments=(table[0], table[1][::-1].copy(), table[2]))
    assert ex.value.code == engine.ERR_PARAM
    check(eng, cols, strand, table, 1, "after the refusals", forms=(form,))


@pytest.mark.parametrize("form", FORMS)
def test_every_refusal_of_the_header(eng, mixed, form):
    from raft_amd import engine
    read_len, table = mixed
    off, fb, fe = table
    cols, strand = make_stream(np.random.default_rng(13), read_len, 300)
    P, L = engine.ERR_PARAM, engine.ERR_TOO_LARGE
    cases = [("min_len 0", P, dict(min_len=0)), ("min_len -1", P, dict(min_len=-1)), ("n_rec -1", P, dict(n_rec=-1)), ("n_reads -1", P, dict(n_reads=-1)),
             ("out_cap -1", P, dict(out_cap=-1, room=8)), ("n_frag -2", P, dict(n_frag=-2)), ("arrays but n_frag -1", P, dict(n_frag=-1)),
             ("n_rec 2^30", L, dict(n_rec=2**30)), ("n_frag 2^31 - 1", L, dict(n_frag=2**31 - 1))]
    for what, code, kw in cases:
        kw.setdefault("out_cap", 100000); kw.setdefault("room", 8)
        rc, err, outs, sm = raw(eng, form, cols, strand, table, **kw)
        assert rc == code and untouched(outs, sm), (what, rc)
    for k in range(6):                                                  # a missing column; the strand
        rc, err, outs, sm = raw(eng, form, cols[:k] + [None] + cols[k + 1:], strand, table, out_cap=100000, room=8)
        assert rc == P and untouched(outs, sm), k
    rc, err, outs, sm = raw(eng, form, cols, None, table, out_cap=100000, room=8)
    assert rc == P and untouched(outs, sm)
    for what, bad in (("no frag_offset", (None, fb, fe)), ("no frag_begin", (off, None, fe)), ("no frag_end", (off, fb, None))):
        rc, err, outs, sm = raw(eng, form, cols, strand, bad, out_cap=100000, room=8, n_reads=read_len.size, n_frag=fb.size)
        assert rc == P and untouched(outs, sm), what
    with pytest.raises(ValueError):
        eng.lift_overlaps(*cols[:5], None, strand, fragments=table)
    with pytest.raises(ValueError):
        eng.lift_overlaps(*cols, strand[:-1], fragments=table)
    check(eng, cols, strand, table, 1, "after the refusals", forms=(form,))


def test_no_reads_no_records_no_rows(eng, mixed):
    read_len, table = mixed
    e, b = np.empty(0, np.int32), np.empty(0, np.uint8)
    check(eng, [e] * 6, b, (np.zeros(1, np.int64), e, e), 1, "no reads")
    check(eng, [e] * 6, b, table, 1, "no records")
    cols, strand = make_stream(np.random.default_rng(14), read_len, 50)
    want = check(eng, cols, strand, (np.zeros(read_len.size + 1, np.int64), e, e), 1, "no rows")
    assert want["n_out"] == 0 and want["records_none"] == 50


# ---- a context's own pass --------------------------------------------------------------------------------------------------------------

def _pass_set():
    """A set whose pass cuts reads into two and three fragments.  -> params, read_len and the six columns"""
    from raft_amd.synth import make_overlaps
    o = make_overlaps(300, seed=5)
    return RaftParams(est_cov=30), [c.numpy() for c in (o.read_len,) + o.columns()]


def test_the_own_pass_and_the_states_of_the_context():
    from raft_amd import engine
    p, pcols = _pass_set()
    read_len = pcols[0]
    want_pass = oracle_run(p, *pcols)
    table = (want_pass["frag_offset"], want_pass["frag_begin"], want_pass["frag_end"])
    cols, strand = make_stream(np.random.default_rng(15), read_len, 1500)
    want = lift(*table, cols, strand)
    eng = engine.Engine(p, device=0)

    def state_error():
        for args in (cols + [strand], on_device(cols + [strand])):
            with pytest.raises(engine.RaftError) as ex:
                eng.lift_overlaps(*args)
            assert ex.value.code == engine.ERR_STATE
        same(eng.lift_overlaps(*cols, strand, fragments=table), want, "explicit arrays in any state")

    state_error()                                                       # no pass at all
    eng.run_host(*pcols)
    s = eng.finish()
    for form in FORMS:
        args = cols + [strand] if form == "host" else on_device(cols + [strand])
        same(eng.lift_overlaps(*args), want, f"own pass, {form} form")
        same(eng.lift_overlaps(*args, min_len=501), lift(*table, cols, strand, 501), f"own pass, {form} form, min_len 501")
    rc, err, outs, sm = raw(eng, "host", cols, strand, OWN, out_cap=0, skip=COLUMNS, n_reads=read_len.size - 1)
    assert rc == engine.ERR_PARAM                                     # n_reads is not the pass's
    got = eng.fetch()
    got.update(symmetric=s.symmetric, high_cov=s.high_cov, total_coverage=s.total_coverage, total_windows=s.total_windows,
               total_repeat_length=s.total_repeat_length, total_read_length=s.total_read_length)
    assert_same_result(got, want_pass, "the pass after the calls")
    eng.set_params(RaftParams(est_cov=30, symmetric_mode=1))            # (three columns go up: the flag is asserted, not detected)
    eng.run_pipelined(*pcols[:4], n_chunks=3)                           # host to host: the context holds no pass afterwards
    state_error()
    eng.close()


def test_inside_a_sequence_on_one_context():
    """pass, filter, lift, pass: the pass's outputs are what they were, and the lift of the filtered stream is the oracle's."""
    from raft_amd import engine
    p, pcols = _pass_set()
    read_len = pcols[0]
    want_pass = oracle_run(p, *pcols)
    table = (want_pass["frag_offset"], want_pass["frag_begin"], want_pass["frag_end"])
    cols, strand = make_stream(np.random.default_rng(16), read_len, 2 * T + 3)
    eng = engine.Engine(p, device=0)

    def full():
        s = eng.finish()
        got = eng.fetch()
        got.update(symmetric=s.symmetric, high_cov=s.high_cov, total_coverage=s.total_coverage, total_windows=s.total_windows,
                   total_repeat_length=s.total_repeat_length, total_read_length=s.total_read_length)
        return got

    eng.run_host(*pcols)
    assert_same_result(full(), want_pass, "the first pass")
    flt = eng.filter_overlaps(*cols, min_span=300)
    keep = (cols[2].astype(np.int64) - cols[1] >= 300) & (cols[5].astype(np.int64) - cols[4] >= 300)
    kept = [c[keep] for c in cols]
    assert flt["n_kept"] == int(keep.sum()) and 0 < flt["n_kept"] < cols[0].size
    got = eng.lift_overlaps(*flt["columns"], strand[keep])
    same(got, lift(*table, kept, strand[keep]), "the kept stream against the own pass")
    assert_same_result({**eng.fetch(), **{k: want_pass[k] for k in ("symmetric", "high_cov", "total_coverage", "total_windows",
                                                                     "total_repeat_length", "total_read_length")}}, want_pass, "the pass behind the lift")
    eng.run_host(*pcols)
    assert_same_result(full(), want_pass, "the second pass")
    same(eng.lift_overlaps(*on_device(kept + [strand[keep]])), lift(*table, kept, strand[keep]), "behind the second pass, device form")
    eng.close()
