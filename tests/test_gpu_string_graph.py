"""GPU: raft_hip_string_graph_device / _host (raft_amd/csrc/string_graph.hpp, string_graph_lib.hip) -- the rows, the survivors, the unitig
table, the edge list, the summary and the error paths -- every output compared in full with the plain-Python rule of
tests/sg_testlib.py; in the device form and the host form, over the sizes at which the kernels change path, the row lengths around
kSgRowLds, layouts whose answer is known, the boundaries of the reducible predicate, and the orders of one stream."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from raft_testlib import ROOT
from sg_testlib import (BEST_SKIPPED, EDGE_COLUMNS, PER_END, RED_U, RED_W, SUMMARY, TABLE, UNPAIRED, contained, layout, oracle, reordered, stream_of)
from test_gpu_overlap_ends import SIZES, STRIDE, T, make_stream, mirrored

from raft_amd.params import RaftParams

pytestmark = pytest.mark.gpu

FORMS = ("device", "host")
ARRAYS = PER_END + TABLE + EDGE_COLUMNS
ROW_LDS = int(re.search(r"^#define RAFT_SG_ROW_LDS (\d+)\b", open(os.path.join(ROOT, "raft_amd", "csrc", "string_graph.hpp")).read(), flags=re.M).group(1))
NO_RECORDS = ([np.zeros(0, np.int32)] * 6, np.zeros(0, np.uint8))


@pytest.fixture(scope="module")
def eng():
    from raft_amd import engine
    e = engine.Engine(RaftParams(est_cov=3), device=0)
    yield e
    e.close()


def given_arrays(form, L, cols, strand, skip, offset=False):
    """-> the eight positional arrays and skip, as the form takes them"""
    import torch
    if form == "host":
        return [L] + list(cols) + [strand], skip

    def dev(a, dt):
        a = np.ascontiguousarray(a)
        if not offset:
            return torch.from_numpy(a).to("cuda:0")
        t = torch.zeros(a.size + 1, dtype=dt, device="cuda:0")[1:]         # 4 bytes (bytes: 1 byte) off a 16-byte line
        t.copy_(torch.from_numpy(a))
        assert a.size == 0 or t.data_ptr() % 16 == (1 if dt == torch.uint8 else 4)
        return t
    return [dev(L, torch.int32)] + [dev(c, torch.int32) for c in cols] + [dev(strand, torch.uint8)], None if skip is None else dev(skip, torch.uint8)


def compare(got, want, tag):
    assert sorted(got) == sorted(ARRAYS + ("n_out", "summary", "kernel_seconds", "launches")), tag
    for k in ARRAYS:
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, k, g.dtype, w.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g.ravel() != w.ravel())
        assert bad.size == 0, f"{tag}: {k} differs at {bad.size} places, first at {bad[0]}: got {g.ravel()[bad[0]]} want {w.ravel()[bad[0]]}"
    assert list(got["summary"]) == SUMMARY and got["summary"] == want["summary"], (tag, got["summary"], want["summary"])
    assert got["n_out"] == want["n_out"] and got["kernel_seconds"] >= 0.0 and got["launches"] >= 0, tag


def check(eng, L, cols, strand, H=1000, F=800, fuzz=1000, symmetric=False, skip=None, emit_removed=False, what="", forms=FORMS, offset=False,
          want=None):
    """Runs the call in every form and compares everything with the oracle (computed once) -> (the wanted dict, the last result)"""
    want = oracle(L, cols, strand, H, F, fuzz, symmetric, skip, emit_removed) if want is None else want
    got = None
    for form in forms:
        tag = f"{what} ({form}, H={H}, F={F}, Z={fuzz}, symmetric={symmetric}, removed={emit_removed}, n_rec={cols[0].size}, n_reads={L.size})"
        arrays, sk = given_arrays(form, L, cols, strand, skip, offset)
        got = eng.string_graph(*arrays, max_overhang=H, min_ratio_permille=F, fuzz=fuzz, symmetric=symmetric, skip=sk, emit_removed=emit_removed)
        compare(got, want, tag)
    return want, got


def alive(want):
    """A case cannot pass on an empty graph: the oracle alone finds a reducible arc and a surviving edge."""
    assert want["summary"]["reducible_arcs"] >= 1 and want["summary"]["kept_edges"] >= 1, want["summary"]


def sized_stream(rng, n_rec):
    """n_rec records: a layout of about that many records (most of them dovetails) and, beyond 60 reads of layout, records of every
    other kind between further reads, the two mixed in one random order."""
    n_layout = int(min(max(n_rec // 4 + 2, 8), 60))
    L, cols, strand, _ = layout(rng, n_layout)
    m = cols[0].size
    if n_rec <= m:
        return (L,) + reordered(cols, strand, np.sort(rng.choice(m, n_rec, replace=False)))
    n_more = 65 if n_rec < STRIDE else 3000
    Lb, cb, sb = make_stream(rng, n_more, n_rec - m, template=rng.integers(2, 8, n_rec - m))
    cb[0] += n_layout
    cb[3] += n_layout
    order = rng.permutation(n_rec)
    return (np.concatenate([L, Lb]),) + reordered([np.concatenate(p) for p in zip(cols, cb)], np.concatenate([strand, sb]), order)


def test_the_header_s_constants():
    from raft_amd import engine
    assert (engine.SG_EDGE_RED_U, engine.SG_EDGE_RED_W, engine.SG_EDGE_UNPAIRED) == (RED_U, RED_W, UNPAIRED) == (1, 2, 4)
    assert engine.SG_EDGE_COLUMNS == EDGE_COLUMNS and BEST_SKIPPED == engine.BEST_SKIPPED
    assert ROW_LDS == 256 and (T, STRIDE) == (1024, 2048 * 1024)


# ---- sizes
@pytest.mark.parametrize("n_rec", SIZES)
def test_every_number_of_records(eng, n_rec):
    rng = np.random.default_rng(n_rec + 5)
    L, cols, strand = sized_stream(rng, n_rec)
    skip = contained(L, cols, strand)
    want, _ = check(eng, L, cols, strand, skip=skip, what="sizes")
    if n_rec >= 63:
        alive(want)
    if n_rec < STRIDE:                                                     # (the grid-stride size once: its oracle takes seconds)
        check(eng, L, cols, strand, fuzz=0, symmetric=True, emit_removed=True, what="sizes", forms=("device",))


@pytest.mark.parametrize("n_reads", [0, 1, 2, 63, 64, 65, 255, 256, 257, 1025])
def test_every_number_of_reads(eng, n_reads):
    rng = np.random.default_rng(n_reads)
    if n_reads >= 2:
        L, cols, strand, _ = layout(rng, n_reads, both=n_reads % 2 == 0) if n_reads <= 257 else layout(rng, 200)
        L = np.concatenate([L, np.full(n_reads - L.size, 7000, np.int32)])             # (1025: reads beyond the layout that nobody names)
    else:
        L, (cols, strand) = np.full(n_reads, 7000, np.int32), NO_RECORDS
    want, _ = check(eng, L, cols, strand, fuzz=0, skip=contained(L, cols, strand) if n_reads else None, what="reads")
    if n_reads >= 63:
        alive(want)
    # ... and without records: empty rows and no edges
    want, got = check(eng, L, *NO_RECORDS, what="no records")
    assert got["n_out"] == 0 and not got["arcs"].any() and not got["kept"].any() and np.all(got["partner"] == -1) and not got["flags"].any()
    assert want["summary"]["ends_dead"] == 2 * n_reads


def arc3to5(q, t, ext, back, length):
    """One record on '+': the 3' end of q against the 5' end of t, the arc q3 -> t5 with that ext and back"""
    return (q, back, length, t, 0, length - ext, 0)


def hub_stream(n_partners, length=60000):
    """Read 0 with n partners staggered along its 3' end, 100 bases apart, and every partner overlapping the next: one row of n arcs, of
    which all but the nearest are reducible at fuzz 0; every other row is short."""
    rows = [arc3to5(0, i, 100 * i, length - 100 * i - 50, length) for i in range(1, n_partners + 1)]
    rows += [arc3to5(i, i + 1, 100, 100, length) for i in range(1, n_partners)]
    return np.full(n_partners + 1, length, np.int32), stream_of(rows)


@pytest.mark.parametrize("row", [0, 1, 2, 63, 64, 65, ROW_LDS - 1, ROW_LDS, ROW_LDS + 1])
def test_every_row_length(eng, row):
    L, (cols, strand) = hub_stream(row)
    order = np.random.default_rng(row).permutation(cols[0].size)
    cols, strand = reordered(cols, strand, order)
    want, got = check(eng, L, cols, strand, H=60000, F=0, fuzz=0, emit_removed=True, what="rows")
    assert want["summary"]["longest_row"] == row and got["arcs"][0, 1] == row
    if row >= 2:
        alive(want)
        assert got["kept"][0, 1] == 1 and want["summary"]["reducible_arcs"] >= row - 1
    # fuzz one short of the spacing is no different; a fuzz of the whole stagger still leaves the nearest
    check(eng, L, cols, strand, H=60000, F=0, fuzz=99, what="rows", forms=("device",))


# ---- layouts whose answer is known
def edge_pairs(res):
    return sorted(tuple(sorted((int(u) >> 1, int(w) >> 1))) for u, w in zip(res["edge_u"], res["edge_w"]))


@pytest.mark.parametrize("seed", [0, 1, 4])
def test_a_linear_layout_keeps_the_consecutive_reads_and_is_one_unitig(eng, seed):
    rng = np.random.default_rng(seed)
    L, cols, strand, slot = layout(rng, 90)
    skip = contained(L, cols, strand)
    want, got = check(eng, L, cols, strand, fuzz=0, skip=skip, what="linear")
    alive(want)
    keep = [int(s) for s in slot if not skip[s]]
    assert edge_pairs(got) == sorted(tuple(sorted(p)) for p in zip(keep[:-1], keep[1:]))
    assert want["summary"]["ends_kept_more"] == 0 and want["summary"]["ends_mutual"] == 2 * (len(keep) - 1)
    for form in FORMS:
        import torch
        to = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")) if form == "device" else (lambda a: a)
        utg = eng.unitigs(to(L), to(got["partner"]), to(got["span"]), to(got["flags"]))
        assert utg["utg_reads"].tolist() == [len(keep)] and not utg["utg_circular"].any()
        assert utg["order"].tolist() in (keep, keep[::-1]) and np.all(utg["unitig"][skip != 0] == -1)


def test_a_circular_layout_is_one_circular_unitig(eng):
    rng = np.random.default_rng(3)
    L, cols, strand, slot = layout(rng, 70, circular=True, length=(10000, 10000))
    want, got = check(eng, L, cols, strand, fuzz=0, what="circular")
    alive(want)
    assert want["summary"]["kept_edges"] == 70 and want["summary"]["ends_mutual"] == 140 and want["summary"]["ends_dead"] == 0
    utg = eng.unitigs(L, got["partner"], got["span"], got["flags"])
    assert utg["utg_reads"].tolist() == [70] and utg["utg_circular"].tolist() == [1]


def test_a_fork_keeps_a_node_with_two_arcs(eng):
    n = 10000
    rows = [arc3to5(i, i + 1, 2000, 2000, n) for i in range(4)] + [arc3to5(0, 2, 4000, 4000, n), arc3to5(1, 3, 4000, 4000, n)]
    rows += [arc3to5(2, 6, 2500, 2500, n), arc3to5(6, 7, 2000, 2000, n), arc3to5(1, 6, 4500, 4500, n)]
    cols, strand = stream_of(rows)
    want, got = check(eng, np.full(8, n, np.int32), cols, strand, fuzz=0, what="fork")
    alive(want)
    assert got["kept"][2, 1] == 2 and got["arcs"][2, 1] == 2 and want["summary"]["ends_kept_more"] == 1
    assert got["partner"][2, 1] == -1 and not got["flags"][2] & 8          # (a fork is no mutual end)
    assert got["partner"][2, 0] == 1 and got["partner"][3, 0] == -1 and got["partner"][6, 0] == -1


# ---- the boundaries of the predicate
def triangle(d_ext, d_back, n=10000):
    """A -> B -> C exact, and A -> C whose ext is off by d_ext and whose back (the ext of its twin) by d_back"""
    return np.full(3, n, np.int32), stream_of([arc3to5(0, 1, 2000, 2000, n), arc3to5(1, 2, 1000, 1000, n), arc3to5(0, 2, 3000 + d_ext, 3000 + d_back, n)])


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("Z", [0, 100])
def test_the_fuzz_on_both_sides_of_the_bound(eng, Z, sign):
    for delta, falls in ((Z, True), (Z + 1, False)):
        L, (cols, strand) = triangle(sign * delta, sign * delta)
        want, got = check(eng, L, cols, strand, fuzz=Z, emit_removed=True, what=f"fuzz {sign * delta}")
        assert want["summary"]["reducible_arcs"] == (2 if falls else 0) and want["summary"]["kept_edges"] == (2 if falls else 3)
        assert got["edge_flags"].tolist() == ([0, RED_U | RED_W, 0] if falls else [0, 0, 0])


def test_an_edge_reducible_from_one_side_only_falls(eng):
    for d_ext, d_back, flag in ((101, 0, RED_W), (0, -101, RED_U)):
        L, (cols, strand) = triangle(d_ext, d_back)
        want, got = check(eng, L, cols, strand, fuzz=100, emit_removed=True, what="one side")
        assert want["summary"]["reducible_arcs"] == 1 and want["summary"]["removed_edges"] == 1
        assert got["edge_flags"].tolist() == [0, flag, 0] and got["kept"][0, 1] == 1 and got["kept"][2, 0] == 1
        _, got = check(eng, L, cols, strand, fuzz=100, what="one side, survivors")
        assert got["n_out"] == 2 and edge_pairs(got) == [(0, 1), (1, 2)]


def test_an_exact_tie_in_ext_removes_neither(eng):
    n = 10000
    # A -> B and A -> C reach equally far and B -> C closes the triangle within the fuzz: under "<=" A -> C would fall.  (C's own side
    # is kept out of it: its path over B is 1100 short of its arc to A.)
    L = np.full(3, n, np.int32)
    cols, strand = stream_of([arc3to5(0, 1, 2000, 2000, n), arc3to5(0, 2, 2000, 3500, n), arc3to5(1, 2, 1, 400, n)])
    want, got = check(eng, L, cols, strand, fuzz=1000, emit_removed=True, what="tie")
    assert not want["reducible"] and got["kept"][0, 1] == 2 and got["edge_flags"].tolist() == [0, 0, 0]
    # ... and one base further it does
    cols, strand = stream_of([arc3to5(0, 1, 2000, 2000, n), arc3to5(0, 2, 2001, 3500, n), arc3to5(1, 2, 1, 400, n)])
    want, got = check(eng, L, cols, strand, fuzz=1000, emit_removed=True, what="tie, one further")
    assert want["reducible"] == {(1, 4)} and got["kept"][0, 1] == 1 and got["edge_flags"].tolist() == [0, RED_U, 0]


def test_two_arcs_that_would_remove_each_other(eng):
    n = 10000
    # A's 3' end reaches B and C equally far; B -> C and C -> B both exist (no layout on a line has that: the rule does not ask)
    cols, strand = stream_of([arc3to5(0, 1, 2000, 6000, n), arc3to5(0, 2, 2000, 6500, n), arc3to5(1, 2, 500, 9000, n), arc3to5(2, 1, 500, 9100, n)])
    want, got = check(eng, np.full(3, n, np.int32), cols, strand, H=10000, F=0, fuzz=1000, emit_removed=True, what="mutual removal")
    assert not {(1, 2), (1, 4)} & want["reducible"] and got["arcs"][0, 1] == 2


# ---- duplicates, symmetry, skip
def test_several_candidates_for_one_arc(eng):
    rng = np.random.default_rng(12)
    L, cols, strand, _ = layout(rng, 120)
    n = cols[0].size
    again = rng.choice(n, n // 2, replace=False)
    extra = [c[again].copy() for c in cols]
    k = rng.choice([0, 3, 50], again.size).astype(np.int32)                # the same record, or one that begins later on the query
    rev = strand[again] != 0
    extra[1] = extra[1] + k
    extra[4] = extra[4] + np.where(rev, 0, k).astype(np.int32)
    extra[5] = extra[5] - np.where(rev, k, 0).astype(np.int32)
    cols = [np.concatenate(p) for p in zip(cols, extra)]
    strand = np.concatenate([strand, strand[again]])
    cols, strand = reordered(cols, strand, rng.permutation(cols[0].size))
    want, _ = check(eng, L, cols, strand, skip=contained(L, cols, strand), fuzz=60, what="duplicates")
    alive(want)
    assert want["summary"]["duplicate_arcs"] > 0 and want["summary"]["unpaired_arcs"] == 0
    check(eng, L, *mirrored(cols, strand), symmetric=True, fuzz=60, emit_removed=True, what="duplicates, mirrored", forms=("device",))


@pytest.mark.parametrize("Z", [0, 1000])
def test_a_mirrored_stream_counted_on_its_query_sides_is_its_half_counted_on_both(eng, Z):
    rng = np.random.default_rng(Z + 2)
    L, cols, strand, _ = layout(rng, 300)
    skip = contained(L, cols, strand)
    half, _ = check(eng, L, cols, strand, fuzz=Z, skip=skip, emit_removed=True, what="half")
    alive(half)
    full, _ = check(eng, L, *mirrored(cols, strand), fuzz=Z, skip=skip, symmetric=True, emit_removed=True, what="mirrored")
    for k in ARRAYS:
        assert np.array_equal(full[k], half[k]), k
    assert full["summary"]["dovetail_views"] == half["summary"]["dovetail_views"] and full["summary"]["unpaired_arcs"] == 0


def test_a_broken_promise_of_symmetry_gives_unpaired_arcs(eng):
    rng = np.random.default_rng(21)
    L, cols, strand, _ = layout(rng, 150)
    want, got = check(eng, L, cols, strand, fuzz=0, symmetric=True, emit_removed=True, what="broken promise")
    assert want["summary"]["unpaired_arcs"] == want["summary"]["arcs"] == want["summary"]["edges"] > 0 and want["summary"]["ends_mutual"] == 0
    assert np.all(got["edge_flags"] & UNPAIRED) and (got["edge_u"] >> 1 > got["edge_w"] >> 1).any()
    check(eng, L, cols, strand, fuzz=0, symmetric=True, what="broken promise, survivors")


def test_every_read_flagged_and_none(eng):
    rng = np.random.default_rng(30)
    L, cols, strand, _ = layout(rng, 100)
    want, got = check(eng, L, cols, strand, skip=np.ones(100, np.uint8), what="all flagged")
    assert want["summary"]["arcs"] == 0 and want["summary"]["views_left_out"] > 0 and want["summary"]["reads_flagged"] == 100
    assert np.all(got["flags"] == BEST_SKIPPED) and want["summary"]["ends_dead"] == 0 and got["n_out"] == 0
    none, _ = check(eng, L, cols, strand, skip=np.zeros(100, np.uint8), what="none flagged")
    alive(none)
    check(eng, L, cols, strand, skip=None, what="no skip", want=none)
    some = (np.arange(100) % 7 == 0).astype(np.uint8) * 200
    alive(check(eng, L, cols, strand, skip=some, what="every seventh")[0])


# ---- the order of the records, the alignment of the columns
def test_five_orders_of_one_stream_give_the_same_bytes(eng):
    rng = np.random.default_rng(77)
    L, cols, strand, _ = layout(rng, 400, both=True)
    skip = contained(L, cols, strand)
    want, first = check(eng, L, cols, strand, skip=skip, fuzz=10, emit_removed=True, what="order 0", forms=("device",))
    alive(want)
    for k in range(1, 6):
        c, s = reordered(cols, strand, rng.permutation(cols[0].size))
        arrays, sk = given_arrays("device", L, c, s, skip)
        got = eng.string_graph(*arrays, skip=sk, fuzz=10, emit_removed=True)
        for name in ARRAYS:
            assert got[name].tobytes() == first[name].tobytes(), (k, name)
        assert got["summary"] == first["summary"], k


@pytest.mark.parametrize("n_rec", [1, 5, 257, 2 * T + 3])
def test_columns_off_the_16_byte_line(eng, n_rec):
    rng = np.random.default_rng(n_rec)
    L, cols, strand = sized_stream(rng, n_rec)
    want, _ = check(eng, L, cols, strand, skip=contained(L, cols, strand), what="misaligned", forms=("device",), offset=True)
    if n_rec >= 63:
        alive(want)


# ---- the entry point itself: capacity, NULL outputs, errors
def raw_call(eng, form, L, cols, strand, skip=None, H=1000, F=800, symmetric=0, fuzz=1000, emit_removed=0, out_cap=0, outs=None, n_reads=None,
             n_rec=None, summary=None):
    """The entry point with the caller's output arrays (eleven, or None: all NULL) -> (code, error_index, n_out, the context's message)"""
    import torch
    from raft_amd import engine
    lib = engine.load_side_library("sg")
    arrays = [L] + list(cols) + [strand, skip]
    if form == "device":
        held = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays]
        eng.use_torch_stream()
        fn = lib.raft_hip_string_graph_device
    else:
        held, fn = arrays, lib.raft_hip_string_graph_host
    p = [engine.M.ptr(a) for a in held]
    err, n_out = C.c_int64(-5), C.c_int64(-7)
    rc = fn(eng._ctx, L.size if n_reads is None else n_reads, p[0], cols[0].size if n_rec is None else n_rec, *p[1:], H, F, symmetric, fuzz,
            emit_removed, out_cap, *[engine.M.ptr(o) for o in (outs or [None] * 11)], C.byref(n_out), None if summary is None else C.byref(summary),
            C.byref(err), None, None)
    return rc, err.value, n_out.value, eng._lib.raft_hip_last_error(eng._ctx).decode()


def marked_outputs(n, cap):
    return ([np.full(2 * n, -9, np.int32) for _ in range(4)] + [np.full(n, 9, np.uint8)] + [np.full(cap, -9, np.int32) for _ in range(5)] +
            [np.full(cap, 9, np.uint8)])


def untouched(outs):
    return all(np.all(o == (9 if o.dtype == np.uint8 else -9)) for o in outs)


def filled(outs, want, tag):
    m = want["n_out"]
    for o, k in zip(outs, ARRAYS):
        w = want[k].ravel()
        assert np.array_equal(o[:w.size], w), (tag, k)
        assert np.all(o[w.size:] == (9 if o.dtype == np.uint8 else -9)), (tag, k, "behind the entries")
    assert m == want["edge_u"].size


@pytest.mark.parametrize("form", FORMS)
def test_the_capacity_one_too_small_and_exact(eng, form):
    from raft_amd import engine
    rng = np.random.default_rng(5)
    L, cols, strand, _ = layout(rng, 200)
    for emit_removed in (0, 1):
        want = oracle(L, cols, strand, fuzz=0, emit_removed=bool(emit_removed))
        alive(want)
        m = want["n_out"]
        outs, sm = marked_outputs(200, m + 3), engine._SgSummary()
        rc, index, n_out, message = raw_call(eng, form, L, cols, strand, fuzz=0, emit_removed=emit_removed, out_cap=m - 1, outs=outs, summary=sm)
        assert rc == engine.ERR_TOO_LARGE and n_out == m and index == -1 and message.startswith("string_graph:"), (rc, n_out, m, message)
        assert untouched(outs) and sm.kept_edges == want["summary"]["kept_edges"]
        rc, index, n_out, _ = raw_call(eng, form, L, cols, strand, fuzz=0, emit_removed=emit_removed, out_cap=m, outs=outs)
        assert rc == engine.OK and n_out == m and index == -1
        filled(outs, want, f"exact, {form}")
    rc, _, _, message = raw_call(eng, form, L, cols, strand, out_cap=-1, outs=marked_outputs(200, 4))
    assert rc == engine.ERR_PARAM and message.startswith("string_graph: out_cap")


@pytest.mark.parametrize("form", FORMS)
def test_every_output_may_be_null(eng, form):
    from raft_amd import engine
    rng = np.random.default_rng(8)
    L, cols, strand, _ = layout(rng, 130)
    want = oracle(L, cols, strand, fuzz=0)
    alive(want)
    sm = engine._SgSummary()
    rc, index, n_out, _ = raw_call(eng, form, L, cols, strand, fuzz=0, summary=sm)
    assert rc == engine.OK and index == -1 and n_out == want["n_out"] and {k: getattr(sm, k) for k in SUMMARY} == want["summary"]
    for only in range(11):
        outs = [None] * 11
        outs[only] = marked_outputs(130, want["n_out"])[only]
        rc, _, _, _ = raw_call(eng, form, L, cols, strand, fuzz=0, out_cap=want["n_out"], outs=outs)
        assert rc == engine.OK and np.array_equal(outs[only], want[ARRAYS[only]].ravel()), ARRAYS[only]


@pytest.mark.parametrize("form", FORMS)
def test_the_first_bad_id_is_reported_and_the_outputs_stay(eng, form):
    from raft_amd import engine
    rng = np.random.default_rng(3)
    n = 6 * T + 3                                                          # (six workgroups)
    L, cols, strand = sized_stream(rng, n)
    n_reads = L.size
    for bad_q, bad_t in (([5500, 700], [900]), ([1500], [40, 6000]), ([n - 1], []), ([], [0]), ([5], [5])):
        c = [x.copy() for x in cols]
        c[0][bad_q] = [n_reads, -1][: len(bad_q)]
        c[3][bad_t] = [-2147483648, n_reads][: len(bad_t)]
        outs, sm = marked_outputs(n_reads, 50), engine._SgSummary(records=-9)
        rc, index, n_out, message = raw_call(eng, form, L, c, strand, out_cap=50, outs=outs, summary=sm)
        assert rc == engine.ERR_READ_ID and index == min(bad_q + bad_t), (form, bad_q, bad_t, rc, index)
        assert message.startswith("string_graph:") and untouched(outs) and sm.records == -9 and n_out == -7
        with pytest.raises(engine.RaftError) as e:
            eng.string_graph(L, *c, strand)
        assert e.value.code == engine.ERR_READ_ID and e.value.index == min(bad_q + bad_t)
    check(eng, L, cols, strand, what="after the bad ids", forms=(form,))


def test_the_refusals(eng):
    from raft_amd import engine
    rng = np.random.default_rng(1)
    L, cols, strand, _ = layout(rng, 65)
    n_rec = cols[0].size
    outs = marked_outputs(65, 10)
    for form in FORMS:
        for kw in ({"H": -1}, {"F": -1}, {"F": 1001}, {"H": -2147483648, "F": 0}, {"fuzz": -1}, {"fuzz": -2147483648}, {"out_cap": -1},
                   {"n_rec": -1}, {"n_reads": -1}):
            rc, _, _, message = raw_call(eng, form, L, cols, strand, outs=outs, **kw)
            assert rc == engine.ERR_PARAM and message.startswith("string_graph:"), (form, kw, rc, message)
        for kw in ({"n_reads": 1 << 30}, {"n_rec": 1 << 30}):
            rc, _, _, message = raw_call(eng, form, L, cols, strand, outs=outs, **kw)
            assert rc == engine.ERR_TOO_LARGE and message.startswith("string_graph:"), (form, kw, rc, message)
        for missing in range(8):
            arrays = [L] + list(cols) + [strand]
            arrays[missing] = None
            rc, _, _, message = raw_call(eng, form, arrays[0], arrays[1:7], arrays[7], outs=outs, n_reads=65, n_rec=n_rec)
            assert rc == engine.ERR_PARAM and message.startswith("string_graph:"), (form, missing)
        assert untouched(outs)
    with pytest.raises(engine.RaftError) as e:
        eng.string_graph(L, *cols, strand, fuzz=-1)
    assert e.value.code == engine.ERR_PARAM and "string_graph" in str(e.value)
    with pytest.raises(ValueError):
        eng.string_graph(L, *cols, None)
    with pytest.raises(ValueError):
        eng.string_graph(L, *cols, strand, skip=np.zeros(64, np.uint8))
    check(eng, L, cols, strand, what="after the refusals")


def test_calls_of_falling_and_rising_size_on_one_context(eng):
    rng = np.random.default_rng(9)
    for n_rec in (4 * T + 1, 5, T + 1, 3, 8 * T + 7, 0, 2 * T):
        L, cols, strand = sized_stream(rng, n_rec)
        want, _ = check(eng, L, cols, strand, skip=contained(L, cols, strand) if n_rec % 2 else None, symmetric=n_rec % 3 == 0, fuzz=n_rec % 5 * 100,
                        emit_removed=n_rec % 2 == 0, what="sequence")
        if n_rec >= 63:
            alive(want)
