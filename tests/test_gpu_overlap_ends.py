"""GPU: raft_hip_overlap_ends_device / _host (raft_amd/csrc/ovl_ends.hpp, ovl_ends_lib.hip) -- the kind of every record, the five
counts and the status of every read, the summary and the error paths -- bit-exact against a vectorised numpy restatement of the rule
of include/raft_hip_end.h; in the device form and the host form, with the kind bytes and without them."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from raft_testlib import ROOT, runs_of

from raft_amd.params import RaftParams

pytestmark = pytest.mark.gpu

FORMS = ("device", "host")
KIND_NAMES = ("kind_invalid", "kind_internal", "kind_query_contained", "kind_target_contained", "kind_end3", "kind_end5", "kind_self")
STATUS_NAMES = ("reads_linked", "reads_contained", "reads_isolated", "reads_dead5", "reads_dead3")


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
    text = open(os.path.join(ROOT, "raft_amd", "csrc", "ovl_ends.hpp")).read()      # launched with the shared ones, no grid of its own
    assert '#include "record_stream.hpp"' in text and "__launch_bounds__(kStreamThreads) void ends_kernel" in text
    assert "_grid(" not in text


# ---- the rule, restated over whole columns (int64 throughout; np.select takes the first condition that holds)
VIEW = np.array([[0, 1, 3, 2, 5, 4, 6], [0, 1, 3, 2, 4, 5, 6]])      # the target's view of a kind on '+' / on '-'
SLOT = np.array([-1, 0, 1, 2, 4, 3, -1])                             # kind -> row of the counts table (internal, contained_in, contains, end5, end3)


def want_kinds(read_len, cols, strand, H, F):
    L = np.asarray(read_len, np.int64)
    qid, qs, qe, tid, ts, te = (np.asarray(c, np.int64) for c in cols)
    lq, lt = L[qid], L[tid]
    rev = np.asarray(strand) != 0
    valid = (0 <= qs) & (qs < qe) & (qe <= lq) & (0 <= ts) & (ts < te) & (te <= lt)
    q5, q3 = qs, lq - qe
    t5, t3 = np.where(rev, lt - te, ts), np.where(rev, ts, lt - te)
    e5, e3, span = np.minimum(q5, t5), np.minimum(q3, t3), np.minimum(qe - qs, te - ts)
    internal = (e5 > H) | (e3 > H) | (span * 1000 < F * (span + e5 + e3))
    qin, tin = (q5 <= t5) & (q3 <= t3), (q5 >= t5) & (q3 >= t3)
    query_loses_tie = np.where(lq != lt, lq < lt, qid > tid)
    return np.select([~valid, qid == tid, internal, qin & tin & query_loses_tie, qin & tin, qin, tin, q5 > t5], [0, 6, 1, 2, 3, 2, 3, 4], default=5).astype(np.uint8)


def want_all(read_len, cols, strand, H, F, symmetric):
    """-> kinds, counts [5, n_reads], status, the summary's counts"""
    n_reads = len(read_len)
    kinds = want_kinds(read_len, cols, strand, H, F) if len(cols[0]) else np.zeros(0, np.uint8)
    flat = np.zeros(5 * n_reads, np.int64)
    sides = [(kinds, np.asarray(cols[0], np.int64))]
    if not symmetric:
        sides.append((VIEW[(np.asarray(strand) != 0).astype(int), kinds], np.asarray(cols[3], np.int64)))
    for k, ids in sides:
        slot = SLOT[k]
        m = slot >= 0
        flat += np.bincount(slot[m] * n_reads + ids[m], minlength=5 * n_reads)
    counts = flat.reshape(5, n_reads).astype(np.int32)
    contained_in, end5, end3 = counts[1], counts[3], counts[4]
    status = np.select([contained_in > 0, (end5 == 0) & (end3 == 0), end5 == 0, end3 == 0], [1, 2, 3, 4], default=0).astype(np.uint8)
    summary = {"n_records": len(kinds)}
    summary.update({n: int((kinds == k).sum()) for k, n in enumerate(KIND_NAMES)})
    summary.update({n: int((status == k).sum()) for k, n in enumerate(STATUS_NAMES)})
    return kinds, counts, status, summary


# ---- streams
def make_stream(rng, n_reads, n_rec, qid=None, tid=None, template=None):
    """Read lengths, six columns and strand bytes: records drawn from eight templates -- dovetails at either end on either strand,
    one read aligned whole inside the other, both aligned whole, matches somewhere inside, invalid coordinates, a read against
    itself -- with overhangs of 0, 1, 2 and up to 1500 bases.  Half of the reads share two lengths (ties by id)."""
    L = rng.integers(5000, 20000, n_reads).astype(np.int32)
    L[::2] = np.where(np.arange(n_reads)[::2] % 4 == 0, 5000, 6000)
    qid = np.sort(rng.integers(0, n_reads, n_rec)) if qid is None else np.asarray(qid)
    tid = rng.integers(0, n_reads, n_rec) if tid is None else np.asarray(tid).copy()
    tpl = rng.integers(0, 8, n_rec) if template is None else np.asarray(template)
    tid = np.where(tpl == 7, qid, tid)
    lq, lt = L[qid].astype(np.int64), L[tid].astype(np.int64)
    jitter = lambda: np.where(rng.random(n_rec) < 0.5, 0, np.where(rng.random(n_rec) < 0.5, rng.integers(1, 3, n_rec), rng.integers(3, 1500, n_rec)))
    j1, j2, ovl = jitter(), jitter(), rng.integers(500, 2500, n_rec)
    rev = rng.integers(0, 2, n_rec).astype(bool)
    qs, qe, ts, te = (np.zeros(n_rec, np.int64) for _ in range(4))

    def put(m, a, b, c, d):
        qs[m], qe[m], ts[m], te[m] = a[m], b[m], c[m], d[m]
    # 0: the query's 3' end against the target's 5' end ('-': against its 3' end)
    put(tpl == 0, lq - j1 - ovl, lq - j1, np.where(rev, lt - j2 - ovl, j2), np.where(rev, lt - j2, j2 + ovl))
    # 1: the query's 5' end
    put(tpl == 1, j1, j1 + ovl, np.where(rev, j2, lt - j2 - ovl), np.where(rev, j2 + ovl, lt - j2))
    # 2 / 3: one read whole (but for the overhangs) somewhere inside the other
    span = np.minimum(lq - j1 - j2, lt)
    at = (rng.random(n_rec) * (lt - span + 1)).astype(np.int64)
    put(tpl == 2, j1, j1 + span, at, at + span)
    span = np.minimum(lt - j1 - j2, lq)
    at = (rng.random(n_rec) * (lq - span + 1)).astype(np.int64)
    put(tpl == 3, at, at + span, j1, j1 + span)
    # 4: both whole
    put(tpl == 4, 0 * lq, lq, 0 * lt, lt)
    # 5: somewhere inside both
    a, b = (rng.random(n_rec) * (lq - 1000)).astype(np.int64), (rng.random(n_rec) * (lt - 1000)).astype(np.int64)
    put(tpl == 5, a, a + ovl % 1000 + 1, b, b + ovl % 1000 + 1)
    # 6: invalid -- empty on the query, beyond the target's end, a negative start, ends before starts
    which = rng.integers(0, 4, n_rec)
    put(tpl == 6, np.where(which == 2, -1, a), np.where(which == 0, a, np.where(which == 3, a - 1, a + 500)), b, np.where(which == 1, lt + 1, b + 500))
    # 7: a read against itself
    put(tpl == 7, 0 * lq, ovl, lq - ovl, lq)
    cols = [c.astype(np.int32) for c in (qid, qs, qe, tid, ts, te)]
    return L, cols, rev.astype(np.uint8)


@pytest.fixture(scope="module")
def eng():
    from raft_amd import engine
    e = engine.Engine(RaftParams(est_cov=3), device=0)
    yield e
    e.close()


def check(eng, L, cols, strand, H=1000, F=800, symmetric=False, what="", forms=FORMS, kinds=(True, False), offset=False, all_kinds=False):
    """Runs the call in every form, with and without the kind bytes, and compares everything with the restatement; -> the wanted tuple."""
    import torch
    n, n_reads = cols[0].size, L.size
    want = want_all(L, cols, strand, H, F, symmetric)
    w_kinds, w_counts, w_status, w_sum = want
    if all_kinds:
        assert all(w_sum[k] > 0 for k in KIND_NAMES), (what, w_sum)
    for form in forms:
        if form == "device":
            def dev(a, dt):
                a = np.ascontiguousarray(a)
                if not offset:
                    return torch.from_numpy(a).to("cuda:0")
                t = torch.zeros(a.size + 1, dtype=dt, device="cuda:0")[1:]     # 4 bytes (strand: 1 byte) off a 16-byte line
                t.copy_(torch.from_numpy(a))
                assert a.size == 0 or t.data_ptr() % 16 == (1 if dt == torch.uint8 else 4)
                return t
            given = [dev(L, torch.int32)] + [dev(c, torch.int32) for c in cols] + [dev(strand, torch.uint8)]
        else:
            given = [L] + list(cols) + [strand]
        for with_kinds in kinds:
            tag = f"{what} ({form}, kinds={with_kinds}, H={H}, F={F}, symmetric={symmetric}, n_rec={n}, n_reads={n_reads})"
            got = eng.overlap_ends(*given, max_overhang=H, min_ratio_permille=F, symmetric=symmetric, kinds=with_kinds)
            assert ("kinds" in got) == with_kinds, tag
            if with_kinds:
                g = got["kinds"].cpu().numpy() if form == "device" else got["kinds"]
                assert g.dtype == np.uint8 and g.shape == w_kinds.shape, tag
                bad = np.flatnonzero(g != w_kinds)
                assert bad.size == 0, f"{tag}: kinds differ at {bad.size} records, first at {bad[0]}: got {g[bad[0]]} want {w_kinds[bad[0]]}"
            assert got["counts"].dtype == np.int32 and got["counts"].shape == (5, n_reads), tag
            bad = np.argwhere(got["counts"] != w_counts)
            assert bad.size == 0, f"{tag}: counts differ at {len(bad)} places, first at {bad[0]}: got {got['counts'][tuple(bad[0])]} want {w_counts[tuple(bad[0])]}"
            assert np.array_equal(got["status"], w_status), tag
            assert {k: got[k] for k in w_sum} == w_sum, (tag, {k: got[k] for k in w_sum}, w_sum)
            assert got["kernel_seconds"] >= 0.0
    return want


@pytest.mark.parametrize("n_rec", SIZES)
def test_every_size(eng, n_rec):
    rng = np.random.default_rng(n_rec + 7)
    L, cols, strand = make_stream(rng, 65, n_rec)
    check(eng, L, cols, strand, what="sizes", all_kinds=n_rec >= 2 * T)


@pytest.mark.parametrize("n_reads", [1, 2, 65, 5000])
def test_every_number_of_reads(eng, n_reads):
    rng = np.random.default_rng(n_reads)
    L, cols, strand = make_stream(rng, n_reads, 2 * T + 3)
    check(eng, L, cols, strand, what="reads", all_kinds=n_reads >= 65)
    check(eng, L, cols, strand, symmetric=True, what="reads", forms=("device",), kinds=(False,))
    L, cols, strand = make_stream(rng, n_reads, 0)
    _, counts, status, summary = check(eng, L, cols, strand, what="no records")
    assert not counts.any() and np.all(status == 2) and summary["reads_isolated"] == n_reads


@pytest.mark.parametrize("F", [0, 800, 1000])
@pytest.mark.parametrize("H", [0, 1, 1000])
def test_every_kind_under_every_parameter(eng, H, F):
    rng = np.random.default_rng(100 * H + F)
    L, cols, strand = make_stream(rng, 65, 4 * T + 1)
    check(eng, L, cols, strand, H=H, F=F, what="parameters", all_kinds=True)
    check(eng, L, cols, strand, H=H, F=F, symmetric=True, what="parameters", forms=("device",), kinds=(True,))


@pytest.mark.parametrize("side", ["query", "target"])
def test_all_records_on_one_read(eng, side):
    rng = np.random.default_rng(5)
    n = 2 * T + 3
    one = np.full(n, 33)
    L, cols, strand = make_stream(rng, 65, n, qid=one if side == "query" else None, tid=one if side == "target" else None,
                                  template=rng.integers(0, 7, n))             # (no record against itself: the column stays one read)
    assert np.all(cols[0 if side == "query" else 3] == 33)
    _, counts, _, _ = check(eng, L, cols, strand, what="one " + side, all_kinds=False)
    assert counts[:, 33].sum() >= n // 2


@pytest.mark.parametrize("lead", [0, 1, 3, 62, 255, T - 1])
def test_runs_across_lane_wave_and_workgroup_edges(eng, lead):
    """Runs of 63 / 64 / 65 / 257 records on one read, begun at every kind of offset, their records alternating between kinds."""
    rng = np.random.default_rng(lead)
    qid = runs_of([63, 64, 65, 257, 1, 2, 257, 65, 64, 63, 5, 257, 4, 4, 4, 3, 1, 1, 256, 1024, 7], first_id=2, lead=lead)
    n = qid.size
    L, cols, strand = make_stream(rng, 65, n, qid=qid, template=np.arange(n) % 6)
    check(eng, L, cols, strand, what="runs, alternating kinds")
    L, cols, strand = make_stream(rng, 65, n, qid=qid, tid=qid[::-1].copy(), template=np.arange(n) % 5)      # (the target column in runs as well)
    check(eng, L, cols, strand, what="runs on both sides", kinds=(True,))
    L, cols, strand = make_stream(rng, 65, n, qid=qid, template=np.zeros(n, int))                            # (one template: long runs of one count)
    check(eng, L, cols, strand, what="runs of one kind", kinds=(False,))


@pytest.mark.parametrize("n_rec", [1, 5, 257, 2 * T + 3])
def test_columns_off_the_16_byte_line(eng, n_rec):
    rng = np.random.default_rng(n_rec)
    L, cols, strand = make_stream(rng, 65, n_rec)
    check(eng, L, cols, strand, what="misaligned", forms=("device",), offset=True)


def mirrored(cols, strand):
    qid, qs, qe, tid, ts, te = cols
    return [np.concatenate(p) for p in ((qid, tid), (qs, ts), (qe, te), (tid, qid), (ts, qs), (te, qe))], np.concatenate((strand, strand))


@pytest.mark.parametrize("H,F", [(1000, 800), (0, 1000), (1, 0)])
def test_a_mirrored_stream_counted_on_its_query_sides_is_its_half_counted_on_both(eng, H, F):
    rng = np.random.default_rng(H + F)
    L, cols, strand = make_stream(rng, 65, 2 * T + 3)
    _, half_counts, half_status, half_sum = check(eng, L, cols, strand, H=H, F=F, what="half", forms=("device",), kinds=(False,))
    full_cols, full_strand = mirrored(cols, strand)
    _, counts, status, summary = check(eng, L, full_cols, full_strand, H=H, F=F, symmetric=True, what="mirrored", kinds=(True,))
    assert np.array_equal(counts, half_counts) and np.array_equal(status, half_status)
    assert all(summary[k] == half_sum[k] for k in STATUS_NAMES)


def raw_call(eng, form, L, cols, strand, H, F, symmetric, counts, status, kinds, n_reads=None, n_rec=None):
    """The entry point itself, with the caller's output arrays -> (code, error_index, the context's message)"""
    import torch
    from raft_amd import engine
    lib = engine.load_side_library("end")
    arrays = [L] + list(cols) + [strand]
    if form == "device":
        held = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays]
        d_kinds = None if kinds is None else torch.from_numpy(kinds).to("cuda:0")
        eng.use_torch_stream()
        fn = lib.raft_hip_overlap_ends_device
    else:
        held, d_kinds, fn = arrays, kinds, lib.raft_hip_overlap_ends_host
    p = [engine.M.ptr(a) for a in held]
    err = C.c_int64(-5)
    rc = fn(eng._ctx, L.size if n_reads is None else n_reads, p[0], cols[0].size if n_rec is None else n_rec, *p[1:], H, F, symmetric,
            engine.M.ptr(counts), engine.M.ptr(status), engine.M.ptr(d_kinds), None, C.byref(err), None)
    return rc, err.value, eng._lib.raft_hip_last_error(eng._ctx).decode()


@pytest.mark.parametrize("form", FORMS)
def test_the_first_bad_id_is_reported_and_the_outputs_stay(eng, form):
    from raft_amd import engine
    rng = np.random.default_rng(3)
    n = 2 * T + 3
    L, cols, strand = make_stream(rng, 65, n)
    for bad_q, bad_t in (([1500, 700], [900]), ([1500], [40, 2000]), ([n - 1], []), ([], [0]), ([5], [5])):
        c = [x.copy() for x in cols]
        c[0][bad_q] = [65, -1][: len(bad_q)]
        c[3][bad_t] = [-2147483648, 65][: len(bad_t)]
        counts, status, kinds = np.full((5, 65), -9, np.int32), np.full(65, 9, np.uint8), np.full(n, 9, np.uint8)
        rc, index, message = raw_call(eng, form, L, c, strand, 1000, 800, 0, counts, status, kinds)
        assert rc == engine.ERR_READ_ID and index == min(bad_q + bad_t), (form, bad_q, bad_t, rc, index)
        assert "overlap_ends" in message
        assert np.all(counts == -9) and np.all(status == 9)
        if form == "host":
            assert np.all(kinds == 9)
        with pytest.raises(engine.RaftError) as e:
            eng.overlap_ends(L, *c, strand)
        assert e.value.code == engine.ERR_READ_ID and e.value.index == min(bad_q + bad_t)
    rc, index, _ = raw_call(eng, form, L, cols, strand, 1000, 800, 0, counts, status, kinds)
    assert rc == engine.OK and index == -1 and np.array_equal(counts, want_all(L, cols, strand, 1000, 800, False)[1])


def test_calls_of_falling_and_rising_size_on_one_context(eng):
    rng = np.random.default_rng(9)
    for n_reads, n_rec in ((5000, 4 * T + 1), (2, 5), (65, T + 1), (1, 3), (5000, 8 * T + 7), (65, 0), (5000, 2 * T)):
        L, cols, strand = make_stream(rng, n_reads, n_rec)
        check(eng, L, cols, strand, what="sequence", symmetric=n_rec % 2 == 0)


def test_the_refusals(eng):
    from raft_amd import engine
    rng = np.random.default_rng(1)
    L, cols, strand = make_stream(rng, 65, 100)
    counts, status = np.full((5, 65), -9, np.int32), np.full(65, 9, np.uint8)
    for form in FORMS:
        for H, F in ((-1, 800), (1000, -1), (1000, 1001), (-2147483648, 0)):
            rc, _, message = raw_call(eng, form, L, cols, strand, H, F, 0, counts, status, None)
            assert rc == engine.ERR_PARAM and message.startswith("overlap_ends:"), (form, H, F, rc, message)
        for kw in ({"n_rec": -1}, {"n_reads": -1}):
            rc, _, message = raw_call(eng, form, L, cols, strand, 1000, 800, 0, counts, status, None, **kw)
            assert rc == engine.ERR_PARAM and message.startswith("overlap_ends:"), (form, kw)
        for missing in range(8):
            arrays = [L] + list(cols) + [strand]
            arrays[missing] = None
            rc, _, message = raw_call(eng, form, arrays[0], arrays[1:7], arrays[7], 1000, 800, 0, counts, status, None, n_reads=65, n_rec=100)
            assert rc == engine.ERR_PARAM and message.startswith("overlap_ends:"), (form, missing)
        assert np.all(counts == -9) and np.all(status == 9)
    with pytest.raises(engine.RaftError) as e:
        eng.overlap_ends(L, *cols, strand, max_overhang=-1)
    assert e.value.code == engine.ERR_PARAM and "overlap_ends" in str(e.value)
    with pytest.raises(ValueError):
        eng.overlap_ends(L, *cols, None)
    check(eng, L, cols, strand, what="after the refusals")
