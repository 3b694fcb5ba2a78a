"""GPU: raft_hip_best_overlaps_device / _host (raft_amd/csrc/best_ovl.hpp, best_ovl_lib.hip) -- per read end the partner, the span and
the strand of the best overlap, whether it is mutual, the flag bytes, the summary and the error paths -- bit-exact against a numpy
restatement of the rule of include/raft_hip_best.h (``np.maximum.at`` over uint64 keys), in the device form and the host form."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from raft_testlib import ROOT, runs_of
from test_gpu_overlap_ends import make_stream, mirrored, want_all, want_kinds

from raft_amd.params import RaftParams

pytestmark = pytest.mark.gpu

FORMS = ("device", "host")
SUMMARY = ("n_records", "candidates", "left_out", "ends_best", "ends_mutual", "reads_both_best", "reads_both_mutual", "reads_no_best", "reads_skipped")
CLASSES = ("slots", "mutual", "both_mutual", "reverse", "left_out", "changed_by_mask")


def _constant(header, name):
    text = open(os.path.join(ROOT, "raft_amd", "csrc", header)).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


# T: the records one workgroup takes per step (record_stream.hpp: kStreamThreads lanes of kStreamLaneRecords records each); beyond
# kStreamMaxBlocks workgroups the grid strides
T = _constant("record_stream.hpp", "kStreamThreads") * _constant("record_stream.hpp", "kStreamLaneRecords")
STRIDE = T * _constant("record_stream.hpp", "kStreamMaxBlocks")
SIZES = [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 3, STRIDE + 2 * T + 5]


def test_the_constants_are_the_expected_ones():
    assert (T, STRIDE) == (1024, 2048 * 1024)
    shared = open(os.path.join(ROOT, "raft_amd", "csrc", "record_stream.hpp")).read()
    assert "const long long per_step = (long long)kStreamThreads * kStreamLaneRecords;" in shared
    text = open(os.path.join(ROOT, "raft_amd", "csrc", "best_ovl.hpp")).read()      # launched with the shared ones, no grid of its own
    assert '#include "record_stream.hpp"' in text and "__launch_bounds__(kStreamThreads) void best_kernel" in text
    assert "_grid(" not in text


# ---- the rule, restated over whole columns
VIEW = np.array([[0, 1, 3, 2, 5, 4, 6], [0, 1, 3, 2, 4, 5, 6]])      # the target's view of a kind on '+' / on '-'
END_OF = np.array([-1, -1, -1, -1, 1, 0, -1])                        # kind -> the end of the viewing read (5: its 5' end, 4: its 3' end)


def want_table(read_len, cols, strand, H, F, symmetric, skip):
    """-> the uint64 keys [2 * n_reads], candidates, left_out (both in views)"""
    n_reads = len(read_len)
    tab = np.zeros(2 * n_reads, np.uint64)
    if len(cols[0]) == 0:
        return tab, 0, 0
    kinds = want_kinds(read_len, cols, strand, H, F).astype(np.int64)
    qid, qs, qe, tid, ts, te = (np.asarray(c, np.int64) for c in cols)
    rev = (np.asarray(strand) != 0).astype(np.int64)
    flagged = np.zeros(n_reads, bool) if skip is None else np.asarray(skip) != 0
    span = np.minimum(qe - qs, te - ts)
    candidates = left_out = 0
    views = [(kinds, qid, tid)] + ([] if symmetric else [(VIEW[rev, kinds], tid, qid)])
    for kind, me, other in views:
        end = END_OF[kind]
        dovetail = end >= 0
        out = dovetail & (flagged[me] | flagged[other])
        m = dovetail & ~out
        left_out += int(out.sum())
        candidates += int(m.sum())
        key = (span[m].astype(np.uint64) << np.uint64(33)) | ((np.uint64(0x7FFFFFFF) - other[m].astype(np.uint64)) << np.uint64(2)) | (rev[m].astype(np.uint64) << np.uint64(1))
        np.maximum.at(tab, 2 * me[m] + end[m], key)
    return tab, candidates, left_out


def want_best(read_len, cols, strand, H, F, symmetric, skip):
    """-> partner [n_reads, 2], span [n_reads, 2], flags, the summary's counts"""
    n_reads = len(read_len)
    tab, candidates, left_out = want_table(read_len, cols, strand, H, F, symmetric, skip)
    have = (tab != 0).reshape(n_reads, 2)
    span = (tab >> np.uint64(33)).astype(np.int64).reshape(n_reads, 2)
    partner = np.where(have, 0x7FFFFFFF - ((tab >> np.uint64(2)) & np.uint64(0x7FFFFFFF)).astype(np.int64).reshape(n_reads, 2), -1)
    rev = ((tab >> np.uint64(1)) & np.uint64(1)).astype(np.int64).reshape(n_reads, 2)
    end = np.broadcast_to(np.arange(2), (n_reads, 2))
    their_end = np.where(rev == 1, end, 1 - end)
    safe = np.where(have, partner, 0)
    back_have, back_partner, back_rev = have[safe, their_end], partner[safe, their_end], rev[safe, their_end]
    mutual = have & back_have & (back_partner == np.arange(n_reads)[:, None]) & (np.where(back_rev == 1, their_end, 1 - their_end) == end)
    skipped = np.zeros(n_reads, bool) if skip is None else np.asarray(skip) != 0
    flags = (rev[:, 0] * 1 + mutual[:, 0] * 2 + rev[:, 1] * 4 + mutual[:, 1] * 8 + skipped * 16).astype(np.uint8)
    n_best, n_mutual = have.sum(axis=1), mutual.sum(axis=1)
    summary = dict(n_records=len(cols[0]), candidates=candidates, left_out=left_out, ends_best=int(have.sum()), ends_mutual=int(mutual.sum()),
                   reads_both_best=int((n_best == 2).sum()), reads_both_mutual=int((n_mutual == 2).sum()),
                   reads_no_best=int((~skipped & (n_best == 0)).sum()), reads_skipped=int(skipped.sum()))
    return partner.astype(np.int32), span.astype(np.int32), flags, summary


def status_mask(read_len, cols, strand, H, F, symmetric):
    """overlap_ends' status == contained as the skip bytes: what the CLI passes"""
    return (want_all(read_len, cols, strand, H, F, symmetric)[2] == 1).astype(np.uint8)


@pytest.fixture(scope="module")
def eng():
    from raft_amd import engine
    e = engine.Engine(RaftParams(est_cov=3), device=0)
    yield e
    e.close()


def check(eng, L, cols, strand, H=1000, F=800, symmetric=False, skip=None, what="", forms=FORMS, offset=False, tally=None):
    """Runs the call in every form and compares everything with the restatement; -> the wanted tuple.  ``tally`` (a dict over CLASSES) takes
    what the case holds of every class."""
    import torch
    n, n_reads = cols[0].size, L.size
    want = want_best(L, cols, strand, H, F, symmetric, skip)
    w_partner, w_span, w_flags, w_sum = want
    # the invariants of the rule, on the restatement itself
    assert w_sum["ends_mutual"] % 2 == 0, what
    for e in range(2):
        for r in np.flatnonzero(w_flags & (2 << (2 * e))):
            p, rev = w_partner[r, e], (w_flags[r] >> (2 * e)) & 1
            pe = e if rev else 1 - e
            assert w_partner[p, pe] == r and w_flags[p] & (2 << (2 * pe)) and ((w_flags[p] >> (2 * pe)) & 1) == rev, (what, r, e)
    if tally is not None:
        tally["slots"] += w_sum["ends_best"]
        tally["mutual"] += w_sum["ends_mutual"]
        tally["both_mutual"] += w_sum["reads_both_mutual"]
        tally["reverse"] += int(((w_flags & 1) != 0).sum() + ((w_flags & 4) != 0).sum())
        tally["left_out"] += w_sum["left_out"]
        if skip is not None:
            plain = want_best(L, cols, strand, H, F, symmetric, None)
            tally["changed_by_mask"] += int(((plain[0] != w_partner) | (plain[1] != w_span)).sum())
    for form in forms:
        if form == "device":
            def dev(a, dt):
                a = np.ascontiguousarray(a)
                if not offset:
                    return torch.from_numpy(a).to("cuda:0")
                t = torch.zeros(a.size + 1, dtype=dt, device="cuda:0")[1:]     # 4 bytes (strand, skip: 1 byte) off a 16-byte line
                t.copy_(torch.from_numpy(a))
                assert a.size == 0 or t.data_ptr() % 16 == (1 if dt == torch.uint8 else 4)
                return t
            given = [dev(L, torch.int32)] + [dev(c, torch.int32) for c in cols] + [dev(strand, torch.uint8)]
            g_skip = None if skip is None else dev(skip, torch.uint8)
        else:
            given, g_skip = [L] + list(cols) + [strand], skip
        tag = f"{what} ({form}, H={H}, F={F}, symmetric={symmetric}, skip={'no' if skip is None else int(np.count_nonzero(skip))}, n_rec={n}, n_reads={n_reads})"
        got = eng.best_overlaps(*given, max_overhang=H, min_ratio_permille=F, symmetric=symmetric, skip=g_skip)
        for key, w in (("partner", w_partner), ("span", w_span)):
            assert got[key].dtype == np.int32 and got[key].shape == (n_reads, 2), tag
            bad = np.argwhere(got[key] != w)
            assert bad.size == 0, f"{tag}: {key} differs at {len(bad)} slots, first at {bad[0]}: got {got[key][tuple(bad[0])]} want {w[tuple(bad[0])]}"
        bad = np.flatnonzero(got["flags"] != w_flags)
        assert got["flags"].dtype == np.uint8 and bad.size == 0, f"{tag}: flags differ at {bad.size} reads, first at {bad[:1]}: got {got['flags'][bad[:1]]} want {w_flags[bad[:1]]}"
        assert {k: got[k] for k in SUMMARY} == w_sum, (tag, {k: got[k] for k in SUMMARY}, w_sum)
        assert got["kernel_seconds"] >= 0.0
    return want


def third(rng, n_reads):
    return (rng.random(n_reads) < 1 / 3).astype(np.uint8)


@pytest.mark.parametrize("n_rec", SIZES)
def test_every_size(eng, n_rec):
    rng = np.random.default_rng(n_rec + 7)
    L, cols, strand = make_stream(rng, 65, n_rec)
    _, _, flags, s = check(eng, L, cols, strand, what="sizes")
    if n_rec == 2 * T + 3:                                 # (as worked out on the CPU beforehand)
        assert s["ends_best"] == 130 and s["ends_mutual"] == 68, s
    check(eng, L, cols, strand, skip=third(rng, 65), what="sizes, a third left out", forms=("device",) if n_rec > STRIDE else FORMS)


@pytest.mark.parametrize("n_reads", [1, 2, 65, 5000])
def test_every_number_of_reads(eng, n_reads):
    n_rec = 2 * T + 3
    rng = np.random.default_rng(n_rec + 7)
    L, cols, strand = make_stream(rng, n_reads, n_rec)
    check(eng, L, cols, strand, what="reads")
    check(eng, L, cols, strand, symmetric=True, what="reads", forms=("device",))
    check(eng, L, cols, strand, skip=third(rng, n_reads), what="reads, a third left out")
    _, _, flags, s = check(eng, L, cols, strand, skip=np.ones(n_reads, np.uint8), what="reads, all left out")
    assert s["ends_best"] == 0 and s["candidates"] == 0 and s["reads_skipped"] == n_reads and np.all(flags == 16)
    if n_reads == 5000:
        mask = status_mask(L, cols, strand, 1000, 800, False)
        _, _, _, s = check(eng, L, cols, strand, skip=mask, what="reads, the contained left out")
        assert (int(mask.sum()), s["ends_best"], s["ends_mutual"]) == (640, 510, 490), s
    L, cols, strand = make_stream(rng, n_reads, 0)
    partner, span, flags, s = check(eng, L, cols, strand, skip=third(rng, n_reads), what="no records")
    assert np.all(partner == -1) and not span.any() and s["ends_best"] == 0 and s["reads_no_best"] + s["reads_skipped"] == n_reads


@pytest.mark.parametrize("F", [0, 800, 1000])
@pytest.mark.parametrize("H", [0, 1, 1000])
def test_every_parameter(eng, H, F):
    rng = np.random.default_rng(100 * H + F)
    L, cols, strand = make_stream(rng, 65, 4 * T + 1)
    for symmetric in (False, True):
        check(eng, L, cols, strand, H=H, F=F, symmetric=symmetric, what="parameters")
        check(eng, L, cols, strand, H=H, F=F, symmetric=symmetric, skip=third(rng, 65), what="parameters, a third left out", forms=("device",))


@pytest.mark.parametrize("side", ["query", "target"])
def test_all_records_on_one_read(eng, side):
    """Every atomic of that side lands on two slots."""
    rng = np.random.default_rng(5)
    n = 2 * T + 3
    one = np.full(n, 33)
    L, cols, strand = make_stream(rng, 65, n, qid=one if side == "query" else None, tid=one if side == "target" else None,
                                  template=rng.integers(0, 7, n))             # (no record against itself: the column stays one read)
    assert np.all(cols[0 if side == "query" else 3] == 33)
    partner, _, _, _ = check(eng, L, cols, strand, what="one " + side)
    assert np.all(partner[33] >= 0)
    check(eng, L, cols, strand, symmetric=True, what="one " + side, forms=("device",))


def dovetails(n_reads, qid, tid, spans, rev, end, length=20000):
    """Clean dovetails of the given spans at the given end (0 / 1) of their queries: reads of one length, no overhang."""
    L = np.full(n_reads, length, np.int32)
    qid, tid, spans, rev, end = (np.asarray(a, np.int64) for a in (qid, tid, spans, rev, end))
    assert np.all(qid != tid) and np.all(spans < length)
    qs, qe = np.where(end == 0, 0, length - spans), np.where(end == 0, spans, length)
    # the query's 5' end meets the target's 3' end on '+', its 5' end on '-'; the query's 3' end the other way round
    t_end = np.where(rev == 1, end, 1 - end)
    ts, te = np.where(t_end == 0, 0, length - spans), np.where(t_end == 0, spans, length)
    return L, [c.astype(np.int32) for c in (qid, qs, qe, tid, ts, te)], rev.astype(np.uint8)


RUNS = [63, 64, 65, 257, 1, 2, 257, 65, 64, 63, 5, 257, 4, 4, 4, 3, 1, 1, 256, 1024, 7]


@pytest.mark.parametrize("lead", [0, 1, 3, 62, 255, T - 1])
def test_runs_across_lane_wave_and_workgroup_edges(eng, lead):
    """Runs of 63 / 64 / 65 / 257 ... records on one read, begun at every kind of offset.  In every run one record is the winner of
    each end -- the first, the last or the middle one -- and every other record a candidate of smaller span."""
    rng = np.random.default_rng(lead)
    qid = runs_of(RUNS, first_id=2, lead=lead)
    n, n_reads = qid.size, 2 + len(RUNS) + 1
    starts = np.flatnonzero(np.r_[True, qid[1:] != qid[:-1]])
    lengths = np.diff(np.r_[starts, n])
    for place in ("first", "last", "middle"):
        for tid in (rng.integers(0, 2, n), None):           # a target column of reads 0 and 1, which no query is; then one in runs as well
            if tid is None:
                tid = (qid[::-1] + 1) % n_reads
                tid = np.where(tid == qid, (tid + 1) % n_reads, tid)
            end = np.arange(n) % 2
            spans = rng.integers(500, 5000, n)
            for s, ln in zip(starts, lengths):
                at = {"first": s, "last": s + ln - 1, "middle": s + ln // 2}[place]
                for e in range(2):                          # the winner of end e: the record of that parity nearest to `at` within the run
                    idx = np.arange(s, s + ln)
                    idx = idx[end[idx] == e]
                    if idx.size:
                        spans[idx[np.argmin(np.abs(idx - at))]] = 9000 + e
            L, cols, strand = dovetails(n_reads, qid, tid, spans, rng.integers(0, 2, n), end)
            _, span, _, s = check(eng, L, cols, strand, symmetric=True, what=f"runs, winner {place}", forms=("device",))
            long_runs = np.unique(qid[np.isin(qid, qid[starts[lengths >= 2]])])
            assert np.all(span[long_runs, 0] == 9000) and np.all(span[long_runs, 1] == 9001) and s["candidates"] == n
            check(eng, L, cols, strand, what=f"runs, winner {place}, both sides", forms=("device",) if place != "middle" else FORMS)


def test_ties(eng):
    rng = np.random.default_rng(21)
    n = 2 * T + 3
    # many candidates of one span to different partners: the smallest partner id wins
    qid = np.sort(rng.integers(0, 8, n))
    tid = rng.integers(8, 65, n)
    L, cols, strand = dovetails(65, qid, tid, np.full(n, 3000), rng.integers(0, 2, n), rng.integers(0, 2, n))
    partner, _, _, _ = check(eng, L, cols, strand, symmetric=True, what="ties between partners")
    for r in range(8):
        for e in range(2):
            m = (qid == r) & ((cols[1] == 0) == (e == 0))
            assert partner[r, e] == (tid[m].min() if m.any() else -1)
    check(eng, L, cols, strand, what="ties between partners, both sides")
    # one span and one partner on both strands: '-' wins
    qid, tid = np.sort(rng.integers(0, 30, n)), None
    tid = (qid + 1 + rng.integers(0, 3, n)) % 65
    L, cols, strand = dovetails(65, qid, tid, np.full(n, 2500), rng.integers(0, 2, n), rng.integers(0, 2, n))
    _, _, flags, _ = check(eng, L, cols, strand, symmetric=True, what="ties between strands")
    assert np.any(flags & 5)
    check(eng, L, cols, strand, what="ties between strands, both sides")
    # exact duplicates: every record four times
    L, cols, strand = make_stream(rng, 65, T + 1)
    once = check(eng, L, cols, strand, what="once", forms=("device",))
    cols4, strand4 = [np.tile(c, 4) for c in cols], np.tile(strand, 4)
    four = check(eng, L, cols4, strand4, what="duplicates")
    assert all(np.array_equal(a, b) for a, b in zip(once[:3], four[:3])) and four[3]["candidates"] == 4 * once[3]["candidates"]


@pytest.mark.parametrize("H,F", [(1000, 800), (0, 1000), (1, 0)])
def test_the_table_does_not_depend_on_the_order(eng, H, F):
    rng = np.random.default_rng(H + F)
    L, cols, strand = make_stream(rng, 65, 2 * T + 3)
    skip = third(rng, 65)
    for mask in (None, skip):
        half = check(eng, L, cols, strand, H=H, F=F, skip=mask, what="half", forms=("device",))
        order = rng.permutation(cols[0].size)               # (with it the query column has no runs)
        shuffled = check(eng, L, [c[order] for c in cols], strand[order], H=H, F=F, skip=mask, what="permuted")
        assert all(np.array_equal(a, b) for a, b in zip(half[:3], shuffled[:3])) and half[3] == shuffled[3]
        full_cols, full_strand = mirrored(cols, strand)
        full = check(eng, L, full_cols, full_strand, H=H, F=F, symmetric=True, skip=mask, what="mirrored")
        assert all(np.array_equal(a, b) for a, b in zip(half[:3], full[:3]))
        assert {k: full[3][k] for k in SUMMARY[1:]} == {k: half[3][k] for k in SUMMARY[1:]}


@pytest.mark.parametrize("n_rec", [1, 5, 257, 2 * T + 3])
def test_columns_off_the_16_byte_line(eng, n_rec):
    rng = np.random.default_rng(n_rec)
    L, cols, strand = make_stream(rng, 65, n_rec)
    check(eng, L, cols, strand, skip=third(rng, 65), what="misaligned", forms=("device",), offset=True)
    check(eng, L, cols, strand, what="misaligned", forms=("device",), offset=True)


def test_calls_of_falling_and_rising_size_on_one_context(eng):
    """A table that is not cleared shows up here: reads that had a best overlap in one call have none in the next."""
    rng = np.random.default_rng(9)
    for n_reads, n_rec in ((5000, 4 * T + 1), (2, 5), (65, T + 1), (1, 3), (5000, 8 * T + 7), (65, 0), (5000, 2 * T), (5000, 3)):
        L, cols, strand = make_stream(rng, n_reads, n_rec)
        check(eng, L, cols, strand, what="sequence", symmetric=n_rec % 2 == 0, skip=third(rng, n_reads) if n_rec % 3 == 0 else None)


def raw_call(eng, form, L, cols, strand, skip, H, F, symmetric, partner, span, flags, n_reads=None, n_rec=None, summary=None):
    """The entry point itself, with the caller's output arrays -> (code, error_index, the context's message)"""
    import torch
    from raft_amd import engine
    lib = engine.load_side_library("best")
    arrays = [L] + list(cols) + [strand, skip]
    if form == "device":
        held = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays]
        eng.use_torch_stream()
        fn = lib.raft_hip_best_overlaps_device
    else:
        held, fn = arrays, lib.raft_hip_best_overlaps_host
    p = [engine.M.ptr(a) for a in held]
    err = C.c_int64(-5)
    rc = fn(eng._ctx, L.size if n_reads is None else n_reads, p[0], cols[0].size if n_rec is None else n_rec, *p[1:], H, F, symmetric,
            engine.M.ptr(partner), engine.M.ptr(span), engine.M.ptr(flags), None if summary is None else C.byref(summary), C.byref(err), None)
    return rc, err.value, eng._lib.raft_hip_last_error(eng._ctx).decode()


def outputs(n_reads=65):
    return np.full((n_reads, 2), -9, np.int32), np.full((n_reads, 2), -9, np.int32), np.full(n_reads, 9, np.uint8)


def untouched(partner, span, flags, summary=None):
    return np.all(partner == -9) and np.all(span == -9) and np.all(flags == 9) and (summary is None or summary.n_records == -9)


@pytest.mark.parametrize("form", FORMS)
def test_the_first_bad_id_is_reported_and_the_outputs_stay(eng, form):
    from raft_amd import engine
    rng = np.random.default_rng(3)
    n = 2 * T + 3
    L, cols, strand = make_stream(rng, 65, n)
    skip = third(rng, 65)
    partner, span, flags = outputs()
    for bad_q, bad_t in (([1500, 700], [900]), ([1500], [40, 2000]), ([n - 1], []), ([], [0]), ([5], [5]), ([2000, 64], [64, 3])):
        c = [x.copy() for x in cols]
        c[0][bad_q] = [65, -1][: len(bad_q)]
        c[3][bad_t] = [-2147483648, 65][: len(bad_t)]
        summary = engine._BestSummary(n_records=-9)
        rc, index, message = raw_call(eng, form, L, c, strand, skip, 1000, 800, 0, partner, span, flags, summary=summary)
        assert rc == engine.ERR_READ_ID and index == min(bad_q + bad_t), (form, bad_q, bad_t, rc, index)
        assert message.startswith("best_overlaps:")
        assert untouched(partner, span, flags, summary)
        with pytest.raises(engine.RaftError) as e:
            eng.best_overlaps(L, *c, strand, symmetric=True)
        assert e.value.code == engine.ERR_READ_ID and e.value.index == min(bad_q + bad_t)
    rc, index, _ = raw_call(eng, form, L, cols, strand, skip, 1000, 800, 0, partner, span, flags)
    want = want_best(L, cols, strand, 1000, 800, False, skip)
    assert rc == engine.OK and index == -1 and np.array_equal(partner, want[0]) and np.array_equal(span, want[1]) and np.array_equal(flags, want[2])


def test_the_refusals(eng):
    from raft_amd import engine
    rng = np.random.default_rng(1)
    L, cols, strand = make_stream(rng, 65, 100)
    skip = third(rng, 65)
    partner, span, flags = outputs()
    for form in FORMS:
        for H, F in ((-1, 800), (1000, -1), (1000, 1001), (-2147483648, 0)):
            rc, _, message = raw_call(eng, form, L, cols, strand, skip, H, F, 0, partner, span, flags)
            assert rc == engine.ERR_PARAM and message.startswith("best_overlaps:"), (form, H, F, rc, message)
        for kw in ({"n_rec": -1}, {"n_reads": -1}):
            rc, _, message = raw_call(eng, form, L, cols, strand, skip, 1000, 800, 0, partner, span, flags, **kw)
            assert rc == engine.ERR_PARAM and message.startswith("best_overlaps:"), (form, kw)
        for missing in range(8):
            arrays = [L] + list(cols) + [strand]
            arrays[missing] = None
            rc, _, message = raw_call(eng, form, arrays[0], arrays[1:7], arrays[7], skip, 1000, 800, 0, partner, span, flags, n_reads=65, n_rec=100)
            assert rc == engine.ERR_PARAM and message.startswith("best_overlaps:"), (form, missing)
        assert untouched(partner, span, flags)
        # ... and a good call afterwards, skip == NULL among them
        for mask in (skip, None):
            p, s, f = outputs()
            rc, index, _ = raw_call(eng, form, L, cols, strand, mask, 1000, 800, 0, p, s, f)
            want = want_best(L, cols, strand, 1000, 800, False, mask)
            assert rc == engine.OK and index == -1 and np.array_equal(p, want[0]) and np.array_equal(s, want[1]) and np.array_equal(f, want[2])
    with pytest.raises(engine.RaftError) as e:
        eng.best_overlaps(L, *cols, strand, max_overhang=-1)
    assert e.value.code == engine.ERR_PARAM and "best_overlaps" in str(e.value)
    with pytest.raises(ValueError):
        eng.best_overlaps(L, *cols, None)
    check(eng, L, cols, strand, what="after the refusals")


def test_a_pass_is_fetched_unchanged_behind_the_call():
    """A pass, then best_overlaps, then the fetch of the pass on one context: the pass's outputs equal those of the same sequence
    without the call."""
    import torch
    from raft_amd import engine
    from raft_amd.synth import make_overlaps
    o = make_overlaps(400, coverage=20, seed=11)
    rl, cols = o.read_len.to("cuda:0"), [c.to("cuda:0") for c in o.columns()]
    rng = np.random.default_rng(4)
    strand = rng.integers(0, 2, cols[0].numel()).astype(np.uint8)
    host = [rl.cpu().numpy()] + [c.cpu().numpy() for c in cols]
    fetched = []
    for with_call in (False, True):
        e = engine.Engine(RaftParams(est_cov=20), device=0)
        try:
            e.run_device(rl, *cols)
            if with_call:                                   # (the pass is in flight on the stream)
                got = e.best_overlaps(rl, *cols, torch.from_numpy(strand).to("cuda:0"), skip=torch.from_numpy(third(rng, 400)).to("cuda:0"))
                want = want_best(host[0], host[1:], strand, 1000, 800, False, None)
                assert got["ends_best"] > 0 and got["reads_skipped"] > 0
            summary = e.finish()
            if with_call:                                   # (the host form stages through q_len and q_col)
                again = e.best_overlaps(*host, strand)
                assert np.array_equal(again["partner"], want[0]) and np.array_equal(again["flags"], want[2]) and again["ends_mutual"] > 0
            out = e.fetch()
            fetched.append({k: np.asarray(v) for k, v in out.items() if hasattr(v, "shape")})
        finally:
            e.close()
        fetched[-1]["summary"] = np.array([summary.n_repeats, summary.n_cuts, summary.n_fragments, summary.total_coverage, summary.total_windows])
    assert fetched[0].keys() == fetched[1].keys() and len(fetched[0]) > 3
    for k in fetched[0]:
        assert np.array_equal(fetched[0][k], fetched[1][k]), k


def test_the_cases_hold_every_class():
    """A class that the cases do not fill would make the comparisons say nothing about it: the streams of test_every_size up to
    2T + 3 records and of test_every_number_of_reads, made again and counted without a call (no form), each hold every class."""
    for n_reads in (65, 5000):
        tally = dict.fromkeys(CLASSES, 0)
        n_rec = 2 * T + 3
        rng = np.random.default_rng(n_rec + 7)
        L, cols, strand = make_stream(rng, n_reads, n_rec)
        check(None, L, cols, strand, forms=(), tally=tally)
        check(None, L, cols, strand, skip=third(rng, n_reads), forms=(), tally=tally)
        assert all(tally[c] > 0 for c in CLASSES), (n_reads, tally)
