"""GPU: raft_hip_filter_overlaps_device / _host (raft_amd/csrc/filter.hpp, filter_lib.hip) -- the records of a stream that pass a
minimum identity and a minimum span, compacted in their order -- bit-exact against a numpy mask of the rule of
include/raft_hip_flt.h: the six kept columns, n_kept, both below_* counts, first_kept and the symmetric flag of the kept stream; in
the device form, the host form and the host form in place."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from raft_testlib import ROOT, assert_same_result, oracle_run

from raft_amd.params import RaftParams

pytestmark = pytest.mark.gpu

FORMS = ("device", "host", "in place")


def _constant(header, name):
    text = open(os.path.join(ROOT, "raft_amd", "csrc", header)).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


def tile_and_scan():
    """T: the records of a tile (filter.hpp: kFltTile = kFltThreads * kFltLaneRecords, kFltLaneRecords = record_stream.hpp's
    kStreamLaneRecords, by that name or by the one census.hpp has for it); S: the tiles one workgroup of the scan takes
    (device_scan.hpp: kScanTile = kScanThreads * kScanItems)."""
    text = open(os.path.join(ROOT, "raft_amd", "csrc", "filter.hpp")).read()
    assert re.search(r"constexpr int kFltLaneRecords = k(Stream|Census)LaneRecords;", text) and "constexpr int kFltTile = kFltThreads * kFltLaneRecords;" in text
    assert "static_assert(kFltLaneRecords == kStreamLaneRecords" in text and '#include "record_stream.hpp"' in text
    assert "constexpr int kScanTile = kScanThreads * kScanItems;" in open(os.path.join(ROOT, "raft_amd", "csrc", "device_scan.hpp")).read()
    T = _constant("filter.hpp", "kFltThreads") * _constant("record_stream.hpp", "kStreamLaneRecords")
    S = _constant("device_scan.hpp", "kScanThreads") * _constant("device_scan.hpp", "kScanItems")
    return T, S


T, S = tile_and_scan()
SIZES = [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 3, S * T - 1, S * T + 1]
PATTERNS = ("all", "none", "every other", "first", "last", "tile dropped", "1 %", "50 %", "99 %")


def test_the_constants_are_the_expected_ones():
    assert (T, S) == (1024, 2048)


def want_filter(cols, matches, block, P, L):
    """The rule, restated: -> keep mask, identity_ok, span_ok (int64 arithmetic throughout)."""
    qid, qs, qe, tid, ts, te = (np.asarray(c, np.int64) for c in cols)
    n = qid.size
    if P == 0:
        identity_ok = np.ones(n, bool)
    else:
        m, b = np.asarray(matches, np.int64), np.asarray(block, np.int64)
        identity_ok = (b > 0) & (m >= 0) & (m * 1000 >= P * b)
    span_ok = np.ones(n, bool) if L == 0 else ((qe - qs >= L) & (te - ts >= L))
    return identity_ok & span_ok, identity_ok, span_ok


def want_symmetric(kept):
    """chop.hpp:171-184 on the kept columns: some record other than the first mirrors the first."""
    if kept[0].size == 0:
        return 0
    first = [int(c[0]) for c in kept]
    mirror = np.ones(kept[0].size, bool)
    for k in range(6):
        mirror &= kept[k] == first[(k + 3) % 6]
    mirror[0] = False
    return int(mirror.any())


def check(eng, cols, matches, block, P, L, what, forms=FORMS, offset_outputs=False):
    """Runs the filter in every form and compares everything with the numpy restatement; -> the last result."""
    import torch
    cols = [np.ascontiguousarray(c, np.int32) for c in cols]
    n = cols[0].size
    keep, identity_ok, span_ok = want_filter(cols, matches, block, P, L)
    kept = [c[keep] for c in cols]
    got = None
    for form in forms:
        quality = [matches, block]
        out = None
        if form == "device":
            given = [torch.from_numpy(c).to("cuda:0") for c in cols]
            quality = [None if q is None else torch.from_numpy(np.ascontiguousarray(q, np.int32)).to("cuda:0") for q in quality]
            if offset_outputs:
                out = [torch.full((n + 1,), -7, dtype=torch.int32, device="cuda:0")[1:] for _ in range(6)]
        elif form == "in place":
            given = [c.copy() for c in cols]
            out = given
        else:
            given = cols
        got = eng.filter_overlaps(*given, *quality, min_identity_permille=P, min_span=L, out=out)
        tag = f"{what} ({form}, P={P}, L={L}, n_rec={n})"
        assert got["n_kept"] == int(keep.sum()), (tag, got["n_kept"], int(keep.sum()))
        assert got["below_identity"] == int((~identity_ok).sum()) and got["below_span"] == int((~span_ok).sum()), tag
        assert got["first_kept"] == (int(np.flatnonzero(keep)[0]) if keep.any() else -1), tag
        assert len(got["columns"]) == 6
        for k, (g, w) in enumerate(zip(got["columns"], kept)):
            g = g.cpu().numpy() if form == "device" else np.asarray(g)
            assert g.dtype == np.int32 and g.shape == w.shape, (tag, k, g.shape, w.shape)
            bad = np.flatnonzero(g != w)
            assert bad.size == 0, f"{tag}: column {k} differs at {bad.size} of {w.size} kept records, first at {bad[0]}: got {g[bad[0]]} want {w[bad[0]]}"
        assert got["symmetric"] == want_symmetric(kept), tag
        assert got["kernel_seconds"] >= 0.0
        if form == "in place":                            # behind the kept records the arrays are what they were
            for g, c in zip(given, cols):
                assert np.array_equal(g[got["n_kept"]:], c[got["n_kept"]:]), tag
        if form == "device" and out is not None:
            assert all(o.data_ptr() % 16 == 4 for o in out)
    return got


@pytest.fixture(scope="module")
def eng():
    from raft_amd import engine
    e = engine.Engine(RaftParams(est_cov=3), device=0)
    yield e
    e.close()


def keep_pattern(pattern, n, rng):
    idx = np.arange(n)
    if pattern == "all":
        return np.ones(n, bool)
    if pattern == "none":
        return np.zeros(n, bool)
    if pattern == "every other":
        return idx % 2 == 0
    if pattern == "first":
        return idx == 0
    if pattern == "last":
        return idx == n - 1
    if pattern == "tile dropped":                         # one whole tile dropped between two kept ones
        return (idx < T) | (idx >= 2 * T)
    return rng.random(n) < {"1 %": 0.01, "50 %": 0.5, "99 %": 0.99}[pattern]


P0, L0 = 990, 500


def stream_for(keep, rng, n_reads=1000):
    """Columns under (P0, L0) whose keep mask is `keep`: a dropped record fails the identity, the query span, the target span, or
    several of them."""
    n = keep.size
    qid, tid = np.sort(rng.integers(0, n_reads, n)), rng.integers(0, n_reads, n)
    why = rng.integers(1, 8, n) * ~keep                   # bit 0: identity, bit 1: query span, bit 2: target span
    qs, ts = rng.integers(0, 10000, n), rng.integers(0, 10000, n)
    qe = qs + np.where(why & 2, rng.integers(-5, L0, n), rng.integers(L0, 30000, n))
    te = ts + np.where(why & 4, rng.integers(-5, L0, n), rng.integers(L0, 30000, n))
    block = rng.integers(1, 40000, n)
    matches = np.where(why & 1, (block * P0 - 1) // 1000 - rng.integers(0, 3, n), -(-block * P0 // 1000) + rng.integers(0, 3, n))
    matches = np.where(why & 1, np.maximum(matches, -1), np.minimum(matches, block))
    cols = [x.astype(np.int32) for x in (qid, qs, qe, tid, ts, te)]
    got, _, _ = want_filter(cols, matches, block, P0, L0)
    assert np.array_equal(got, keep)
    return cols, matches.astype(np.int32), block.astype(np.int32)


@pytest.mark.parametrize("n_rec", SIZES)
def test_sizes_and_keep_patterns(eng, n_rec):
    rng = np.random.default_rng(1000 + n_rec)
    for pattern in PATTERNS:
        cols, matches, block = stream_for(keep_pattern(pattern, n_rec, rng), rng)
        got = check(eng, cols, matches, block, P0, L0, pattern)
        if pattern == "tile dropped" and n_rec > 2 * T:
            assert got["n_kept"] == n_rec - T


def test_more_tiles_than_the_capped_grid():
    """(the grid is capped at kFltMaxBlocks workgroups, which S * T + 1 records just pass: stated, so that a retune shows)"""
    assert _constant("filter.hpp", "kFltMaxBlocks") * T < SIZES[-1]


@pytest.mark.parametrize("n_rec", [5, 257, T + 1, 2 * T + 3])
def test_columns_offset_by_one_element(eng, n_rec):
    """Device columns that do not begin on 16 bytes take the 4-byte loads; the outputs are offset as well."""
    import torch
    rng = np.random.default_rng(7 + n_rec)
    cols, matches, block = stream_for(keep_pattern("50 %", n_rec + 1, rng), rng)
    dev = [torch.from_numpy(c).to("cuda:0")[1:] for c in cols + [matches, block]]
    assert all(d.data_ptr() % 16 == 4 for d in dev)
    out = [torch.full((n_rec + 1,), -7, dtype=torch.int32, device="cuda:0")[1:] for _ in range(6)]
    keep, identity_ok, span_ok = want_filter([c[1:] for c in cols], matches[1:], block[1:], P0, L0)
    got = eng.filter_overlaps(*dev, min_identity_permille=P0, min_span=L0, out=out)
    assert got["n_kept"] == int(keep.sum()) and got["first_kept"] == int(np.flatnonzero(keep)[0])
    assert got["below_identity"] == int((~identity_ok).sum()) and got["below_span"] == int((~span_ok).sum())
    for g, c in zip(got["columns"], cols):
        assert np.array_equal(g.cpu().numpy(), c[1:][keep])
    # ... the quality columns alone unaligned, and the outputs alone
    aligned = [torch.from_numpy(np.ascontiguousarray(c[1:])).to("cuda:0") for c in cols]
    got = eng.filter_overlaps(*aligned, dev[6], dev[7], min_identity_permille=P0, min_span=L0)
    assert all(np.array_equal(g.cpu().numpy(), c[1:][keep]) for g, c in zip(got["columns"], cols))
    check(eng, [c[1:] for c in cols], matches[1:], block[1:], P0, L0, "offset outputs", forms=("device",), offset_outputs=True)


I31 = 2 ** 31 - 1
EDGES = [
    # matches, block, qs, qe, ts, te                    P     L    keep
    ((I31, I31, 0, 10, 0, 10), 1000, 0, True),          # the products need 64 bits
    ((I31 - 1, I31, 0, 10, 0, 10), 1000, 0, False),
    ((I31 - 1, I31, 0, 10, 0, 10), 999, 0, True),
    ((5, 0, 0, 10, 0, 10), 1, 0, False),                # block = 0 (a ten-field line) fails every P > 0
    ((0, 0, 0, 10, 0, 10), 1, 0, False),
    ((5, 0, 0, 10, 0, 10), 0, 0, True),                 # ... and passes P = 0
    ((-1, 10, 0, 10, 0, 10), 1, 0, False),              # negative matches
    ((-1, -10, 0, 10, 0, 10), 1, 0, False),             # ... over a negative block: no quotient is formed
    ((10, -10, 0, 10, 0, 10), 1, 0, False),
    ((999, 1000, 0, 10, 0, 10), 999, 0, True),          # identity exactly at the threshold
    ((999, 1000, 0, 10, 0, 10), 1000, 0, False),        # ... and one per mille below
    ((1000, 1000, 0, 10, 0, 10), 1000, 0, True),
    ((0, 1, 0, 10, 0, 10), 1, 0, False),
    ((1, 1000, 0, 10, 0, 10), 1, 0, True),
    ((1, 1001, 0, 10, 0, 10), 1, 0, False),
    ((1, 1, 10, 5, 0, 500), 0, 1, False),               # qe < qs
    ((1, 1, 10, 5, 0, 500), 0, 0, True),
    ((1, 1, 100, 600, 7, 507), 0, 500, True),           # both spans exactly L
    ((1, 1, 100, 599, 7, 507), 0, 500, False),          # L - 1 on the query side alone
    ((1, 1, 100, 600, 7, 506), 0, 500, False),          # ... on the target side alone
    ((1, 1, -I31, I31, -I31, I31), 0, I31, True),       # a span beyond 32 bits
    ((1, 1, I31, -I31, 0, I31), 0, 1, False),
    ((1, 1, 0, I31, 0, I31), 0, I31, True),
    ((1, 1, 0, I31 - 1, 0, I31), 0, I31, False),
]


def test_arithmetic_edges(eng):
    for P, L in sorted({(e[1], e[2]) for e in EDGES}):
        rows = [e for e in EDGES if (e[1], e[2]) == (P, L)]
        rows = rows + [EDGES[0]] * 3 + rows[::-1]          # (more than a lane's four records, each edge at two places)
        vals = [np.array([r[0][k] for r in rows], np.int32) for k in range(6)]
        ids = np.arange(len(rows), dtype=np.int32)
        cols = [ids, vals[2], vals[3], ids + 1, vals[4], vals[5]]
        keep, _, _ = want_filter(cols, vals[0], vals[1], P, L)
        said = [bool(r[3]) if (r[1], r[2]) == (P, L) else bool(k) for r, k in zip(rows, keep)]
        assert list(keep) == said, (P, L, list(keep), said)    # the restatement and the table agree
        check(eng, cols, vals[0], vals[1], P, L, "edges")


@pytest.mark.parametrize("n_rec", [1, 5, T + 1])
def test_no_identity_rule_needs_no_quality_columns(eng, n_rec):
    rng = np.random.default_rng(3)
    cols, matches, block = stream_for(keep_pattern("50 %", n_rec, rng), rng)
    a = check(eng, cols, None, None, 0, L0, "no quality columns")
    b = check(eng, cols, matches, block, 0, L0, "quality columns unread")
    assert a["n_kept"] == b["n_kept"] and a["below_identity"] == 0
    got = check(eng, cols, None, None, 0, 0, "no rule at all")
    assert got["n_kept"] == n_rec and got["below_span"] == 0


def test_refusals(eng):
    import torch

    from raft_amd import engine
    rng = np.random.default_rng(5)
    cols, matches, block = stream_for(keep_pattern("50 %", 100, rng), rng)
    dev = [torch.from_numpy(c).to("cuda:0") for c in cols + [matches, block]]

    def refused(call):
        with pytest.raises(engine.RaftError) as e:
            call()
        assert e.value.code == engine.ERR_PARAM and "filter_overlaps" in str(e.value), str(e.value)

    for given in (cols + [matches, block], dev):
        for P, L in ((-1, 0), (1001, 0), (0, -1), (1000, -5)):
            refused(lambda: eng.filter_overlaps(*given, min_identity_permille=P, min_span=L))
        refused(lambda: eng.filter_overlaps(*given[:6], min_identity_permille=1))                       # no quality columns, P > 0
        refused(lambda: eng.filter_overlaps(*given[:7], None, min_identity_permille=1))
        refused(lambda: eng.filter_overlaps(*given[:6], None, given[7], min_identity_permille=1000))
        for k in range(6):                                                                              # a missing column
            refused(lambda: eng.filter_overlaps(*[None if j == k else c for j, c in enumerate(given[:6])], min_span=1))
    # the device form: an output that overlaps an input or another output
    spare = [torch.zeros(100, dtype=torch.int32, device="cuda:0") for _ in range(6)]
    refused(lambda: eng.filter_overlaps(*dev, min_identity_permille=P0, out=dev[:6]))
    refused(lambda: eng.filter_overlaps(*dev, min_identity_permille=P0, out=spare[:5] + [dev[7]]))
    refused(lambda: eng.filter_overlaps(*dev, min_identity_permille=P0, out=spare[:5] + [spare[0]]))
    both = torch.zeros(150, dtype=torch.int32, device="cuda:0")
    refused(lambda: eng.filter_overlaps(*dev, min_identity_permille=P0, out=spare[:4] + [both[:100], both[50:]]))
    # a negative count, and a missing output, reach the library only directly
    flt = engine.load_side_library("flt")
    for fn, given in ((flt.raft_hip_filter_overlaps_host, cols), (flt.raft_hip_filter_overlaps_device, dev)):
        ptrs = [engine.M.ptr(x) for x in given[:6]]
        outs = [engine.M.ptr(x) for x in (spare if given is dev else [np.zeros(100, np.int32) for _ in range(6)])]
        sm = engine._FltSummary()
        assert fn(eng._ctx, -1, *ptrs, None, None, 0, 0, *outs, C.byref(sm), None) == engine.ERR_PARAM
        assert b"filter_overlaps" in eng._lib.raft_hip_last_error(eng._ctx)
        assert fn(eng._ctx, 100, *ptrs, None, None, 0, 0, *outs[:5], None, C.byref(sm), None) == engine.ERR_PARAM
        assert b"filter_overlaps" in eng._lib.raft_hip_last_error(eng._ctx)
    # ... and the context is as good as before
    check(eng, cols, matches, block, P0, L0, "after the refusals")


def test_the_symmetric_flag_of_the_kept_stream(eng):
    def rows_to_cols(rows):
        a = np.array(rows, np.int32)
        return [a[:, k].copy() for k in range(6)], a[:, 6].copy(), a[:, 7].copy()
    good, bad = (990, 1000), (900, 1000)
    first = (3, 100, 900, 8, 50, 850)
    mirror = (8, 50, 850, 3, 100, 900)
    other = (4, 0, 700, 9, 10, 710)
    for pad in (0, 70, T + 5):                            # the mirror in the first record's lane, in another word, in another tile
        filler = [other + good] * pad
        # the unfiltered stream's first record is dropped: the kept stream's first record is `first`
        kept_mirror = [other + bad, first + good] + filler + [mirror + good, other + good]
        dropped_mirror = [other + bad, first + good] + filler + [mirror + bad, other + good]
        got = check(eng, *rows_to_cols(kept_mirror), 950, 0, f"mirror kept, pad {pad}")
        assert got["symmetric"] == 1 and got["first_kept"] == 1
        got = check(eng, *rows_to_cols(dropped_mirror), 950, 0, f"mirror dropped, pad {pad}")
        assert got["symmetric"] == 0 and got["first_kept"] == 1
        # the mirror of the UNFILTERED stream's first record does not count once that record is dropped
        got = check(eng, *rows_to_cols([mirror + bad, first + good] + filler + [other + good, first + good]), 950, 0, f"mirror before, pad {pad}")
        assert got["symmetric"] == 0
        # a self overlap is its own mirror: not symmetric by that record alone, symmetric with a second copy
        own = (5, 10, 500, 5, 10, 500)
        got = check(eng, *rows_to_cols([other + bad, own + good] + filler + [other + good]), 950, 0, f"self overlap, pad {pad}")
        assert got["symmetric"] == 0 and got["first_kept"] == 1
        got = check(eng, *rows_to_cols([other + bad, own + good] + filler + [own + good]), 950, 0, f"self overlap twice, pad {pad}")
        assert got["symmetric"] == 1
        got = check(eng, *rows_to_cols([other + bad, own + good] + filler + [own + bad]), 950, 0, f"self overlap, copy dropped, pad {pad}")
        assert got["symmetric"] == 0


@pytest.mark.parametrize("symmetric", [True, False])
def test_a_pass_and_a_census_on_the_kept_stream(symmetric):
    """run_device on the kept tensors is oracle_run on the numpy-filtered columns; census on the kept stream likewise."""
    import torch

    from raft_amd import engine
    from raft_amd.synth import make_overlaps
    o = make_overlaps(300, coverage=20, seed=11, symmetric=symmetric)
    rl = o.read_len.numpy()
    cols = [c.numpy() for c in o.columns()]
    rng = np.random.default_rng(12)
    block = np.maximum(cols[2] - cols[1], 1).astype(np.int32)
    # a record and its mirror share their identity, as in a real all-vs-all PAF: per mille by the pair of reads, rounded up to matches
    key = np.minimum(cols[0], cols[3]).astype(np.int64) * 2 ** 20 + np.maximum(cols[0], cols[3])
    matches = (-(-block.astype(np.int64) * (960 + (key * 7919 + 13) % 41) // 1000)).astype(np.int32)
    matches[0] = 0                                       # the input's first record goes
    P, L = 980, 1500
    keep, _, _ = want_filter(cols, matches, block, P, L)
    assert 0.2 * keep.size < keep.sum() < 0.8 * keep.size
    kept = [c[keep] for c in cols]
    p = RaftParams(est_cov=12)
    want = oracle_run(p, rl, *kept)
    assert want["symmetric"] == int(symmetric) and not keep[0]          # (the kept stream begins with another record than the input)
    eng = engine.Engine(p, device=0)
    try:
        dev = [torch.from_numpy(c).to("cuda:0") for c in cols + [matches, block]]
        got = eng.filter_overlaps(*dev, min_identity_permille=P, min_span=L)
        assert got["n_kept"] == int(keep.sum()) and got["symmetric"] == want["symmetric"]
        d_rl = o.read_len.to("cuda:0")
        eng.run_device(d_rl, *got["columns"])
        s = eng.finish()
        res = eng.fetch()
        res.update(symmetric=s.symmetric, high_cov=s.high_cov, total_coverage=s.total_coverage, total_windows=s.total_windows,
                   total_repeat_length=s.total_repeat_length, total_read_length=s.total_read_length)
        assert_same_result(res, want, f"the kept stream (symmetric={symmetric})")
        assert s.n_records == int(keep.sum())
        a = eng.census(d_rl, *got["columns"], symmetric=False)
        b = eng.census(rl, *kept, symmetric=False)
        assert np.array_equal(a["intervals"], b["intervals"]) and np.array_equal(a["contained"], b["contained"]) and a["n_contained"] == b["n_contained"]
        # ... and the same through the host form
        host = eng.filter_overlaps(*cols, matches, block, min_identity_permille=P, min_span=L)
        assert all(np.array_equal(g, w) for g, w in zip(host["columns"], kept))
        eng.run_host(rl, *host["columns"])
        s2 = eng.finish()
        assert s2.total_coverage == s.total_coverage and s2.n_fragments == s.n_fragments and s2.symmetric == s.symmetric
    finally:
        eng.close()


def test_two_filters_a_pass_and_a_query_on_one_context():
    """The host forms share one staging set (q_col): nothing of an earlier call may show in a later one."""
    from raft_amd import engine
    from raft_amd.synth import make_overlaps
    o = make_overlaps(300, coverage=20, seed=21, symmetric=False)
    rl = o.read_len.numpy()
    cols = [c.numpy() for c in o.columns()]
    rng = np.random.default_rng(22)
    block = np.maximum(cols[2] - cols[1], 1).astype(np.int32)
    matches = (block.astype(np.int64) * rng.integers(950, 1001, block.size) // 1000).astype(np.int32)
    eng = engine.Engine(RaftParams(est_cov=12), device=0)
    try:
        eng.run_host(rl, *cols)
        s = eng.finish()
        before = eng.repeat_stats(rl, *cols)
        first = check(eng, cols, matches, block, 990, 0, "first filter", forms=("host",))
        small = [c[: T + 7] for c in cols]
        second = check(eng, small, matches[: T + 7], block[: T + 7], 0, 2000, "second filter, fewer records", forms=("host", "device"))
        assert second["n_kept"] < first["n_kept"]
        eng.run_host(rl, *cols)
        s2 = eng.finish()
        assert s2.total_coverage == s.total_coverage and s2.n_repeats == s.n_repeats
        after = eng.repeat_stats(rl, *cols)
        for k, v in before.items():
            assert np.array_equal(np.asarray(v), np.asarray(after[k])), k
        third = check(eng, cols, matches, block, 990, 0, "the first filter again, after a query", forms=("host", "in place"))
        assert third["n_kept"] == first["n_kept"]
        kept = eng.repeat_stats(rl, *third["columns"])     # a query on the kept stream right behind the filter that made it
        keep, _, _ = want_filter(cols, matches, block, 990, 0)
        fresh = eng.repeat_stats(rl, *[c[keep] for c in cols])
        for k, v in fresh.items():
            assert np.array_equal(np.asarray(v), np.asarray(kept[k])), k
    finally:
        eng.close()
