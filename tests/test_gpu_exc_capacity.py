"""GPU: every exception list at its capacity -- one entry below, exactly full, one entry too many -- on every route that fills one
(the sets of raft_testlib exc_capacity_cases; what they hold and that they hold it: tests/test_exc_capacity_cases.py).

The other suites overflow the lists by thousands of entries; here the number of listed windows K sits on the list's first size
cap0, where `<` and `<=` differ:
    a pass in the set's width (1 / 2)     the pileup kernels fill the list (pack.hpp pack_note); raft_hip_finish runs the pass again
                                          exactly when K > cap0 (engine.hip rerun_ladder), and never on the context's second pass
    an int32 pass, fetched in a width     pack_coverage (engine.hip) fills it, once more with room when K > cap
    a pass that writes four-bit steps     lists every tile's first window too: the read count is swept across cap0 instead
    the fetches as the ABI has them       size query, exc_cap = n - 1 / n / n + 1 (fetch_packed_impl)
    the host pipelines                    the caller's exc_cap at 0, a first chunk's share, E - 1, E, E + 1 (engine_pipeline.hip)
Bit-exact against the oracle and the sets' closed forms.  A fresh context per case: a context's capacity only grows."""
import ctypes as C
import functools

import numpy as np
import pytest
from raft_testlib import (EXC_CAP_FLOOR, EXC_COLD_W, EXC_LIMIT, KERNELS, RaftParams, assert_same_result, exc_capacity_case, exc_capacity_list,
                          exc_case_id, exc_classes, exc_closed_list, exc_steps_set, kernel_mode, oracle_run)
from test_gpu_deep import RERUN
from test_gpu_delta4 import check_encoding, check_pipelined_d4, result_of
from test_gpu_lattice import runner
from test_gpu_packed_output import decode

pytestmark = pytest.mark.gpu

BOUNDARY, SMALL = exc_capacity_list(), exc_capacity_list("small")
PASS_SPECS = [s for s in BOUNDARY if any(c[1] == "pass" for c in exc_classes(s[0], s[2], s[3]))]
REENCODE_SPECS = [s for s in BOUNDARY if any(c[1] == "reencode" for c in exc_classes(s[0], s[2], s[3]))]
FORMS = ("columns", "grouped")
MARK = -77


@functools.lru_cache(maxsize=2)
def built(spec):
    """The set and the oracle's result, made once per set and shared by the tests that follow one another on it."""
    case = exc_capacity_case(*spec)
    want = case.oracle()
    for a in want.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case, want


def check_list(f, case, want, what):
    """A fetched encoding of widths 1 / 2: the codes, and exactly the closed-form list, ascending, with the true values."""
    limit = EXC_LIMIT[case.width]
    assert f["cov8"].dtype == (np.uint8 if case.width == 1 else np.uint16), what
    assert np.array_equal(f["cov8"], np.minimum(want["cov"], limit)), what
    assert f["exc_index"].size == case.K and np.array_equal(f["exc_index"], case.expect), (what, f["exc_index"].size, case.K)
    assert np.array_equal(f["exc_value"], want["cov"][case.expect]), what
    for k in ("cov_offset", "rep_offset", "rep_s", "rep_e", "frag_offset", "frag_read", "frag_begin", "frag_end"):
        assert np.array_equal(f[k], want[k]), (what, k)


def check_device_list(eng, case, want, what):
    """packed_device(): the list as the pass left it on the device, in no particular order."""
    pk = eng.packed_device()
    assert pk is not None and pk["width"] == case.width, what
    xi, xv = pk["exc_index"].cpu().numpy(), pk["exc_value"].cpu().numpy()
    order = np.argsort(xi, kind="stable")
    assert xi.size == case.K and np.array_equal(xi[order], case.expect) and np.array_equal(xv[order], want["cov"][case.expect]), (what, xi.size, case.K)


# ---- 2. one context: the pass's own re-run and the re-encode ---------------------------------------------------------------------------

@pytest.mark.parametrize("spec", PASS_SPECS, ids=exc_case_id)
@pytest.mark.parametrize("kernel", KERNELS)
def test_pass_in_the_sets_width(spec, kernel):
    """K = cap0 - 1, cap0: the list holds them, nothing is run again.  K = cap0 + 1: the first pass counts one more than it lists and
    is run again with room for exactly K; the context's second pass over the set has the room and is not."""
    from raft_amd import engine
    case, want = built(spec)
    cap0 = case.cap0("pass")
    assert abs(case.K - cap0) <= 1
    with kernel_mode(kernel):
        for form in FORMS:
            eng = engine.Engine(case.p, device=0)
            try:
                eng.set_output_width(case.width)
                run = runner(eng, case, form)
                for it in range(2):
                    what = f"set {case.name}, form {form}, kernel {kernel}, pass {it} (cap0 {cap0})"
                    s = run()
                    assert bool(s.flags & RERUN) == (it == 0 and case.K > cap0), (what, s.flags)
                    check_device_list(eng, case, want, what)
                    check_list(eng.fetch_packed(width=case.width), case, want, what)
                    assert_same_result(result_of(eng, s), want, what + ": int32 decoded on the device")
            finally:
                eng.close()


@pytest.mark.parametrize("spec", REENCODE_SPECS, ids=exc_case_id)
@pytest.mark.parametrize("kernel", KERNELS)
def test_int32_pass_encoded_afterwards(spec, kernel):
    """pack_coverage on either side of its cap: one or two bytes start at max(4096, B / 512), four-bit steps at max(4096, B / 64); a
    list one entry longer is made a second time with room for exactly K."""
    from raft_amd import engine
    case, want = built(spec)
    assert abs(case.K - case.cap0("reencode")) <= 1
    with kernel_mode(kernel):
        for form in FORMS:
            eng = engine.Engine(case.p, device=0)
            try:
                eng.set_output_width(4)
                run = runner(eng, case, form)
                for it in range(2):
                    what = f"set {case.name}, form {form}, kernel {kernel}, pass {it} (cap0 {case.cap0('reencode')})"
                    s = run()
                    if kernel == "wave":                   # (an int32 pass has no list to overflow; with every tile the deep kernel's, ITS list may)
                        assert not (s.flags & RERUN), (what, s.flags)
                    assert eng.packed_device() is None, what
                    if case.width == 8:
                        d4 = eng.fetch_delta4()
                        check_encoding(d4, want, what)
                        assert d4["exc_index"].size == case.K and np.array_equal(d4["exc_index"], case.expect), (what, d4["exc_index"].size)
                    else:
                        check_list(eng.fetch_packed(width=case.width), case, want, what)
                        check_device_list(eng, case, want, what)
                    assert_same_result(result_of(eng, s), want, what + ": int32 after the encoding was made")
            finally:
                eng.close()


SWEEP_TILE = 1000
SWEEP_B = EXC_CAP_FLOOR + 2 + 2 * EXC_COLD_W


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_pass_that_writes_four_bit_steps_swept_across_the_first_size(kernel, form):
    """The kernel lists the windows whose step leaves +-7 AND every tile's first window: the total is no closed form of the data.  The
    number of alternating one-window reads runs from 40 below the first size to 2 above it.  A tile ends with 63 reads, a long read
    or a range of 1000 windows, so most first windows are large steps already and a handful (the cold reads') come on top: the
    totals pass through cap0 and cap0 + 1 -- asserted --, and the pass is run again exactly from cap0 + 1 on."""
    from raft_amd import engine
    cap0 = max(EXC_CAP_FLOOR, SWEEP_B // 64)
    assert cap0 == EXC_CAP_FLOOR
    seen = {}
    with kernel_mode(kernel):
        for n_alt in range(cap0 - 40, cap0 + 3):
            case = exc_steps_set(n_alt, SWEEP_B)
            want = case.oracle()
            eng = engine.Engine(case.p, device=0)
            try:
                eng.set_tuning(SWEEP_TILE, False, -1)
                eng.set_output_width(8)
                s = runner(eng, case, form)()
                what = f"{n_alt} alternating reads, form {form}, kernel {kernel}"
                pk = eng.packed_device()
                assert pk is not None and pk["width"] == 8, what
                d4 = eng.fetch_delta4()
                check_encoding(d4, want, what)
                n = int(d4["exc_index"].size)
                assert n == int(pk["exc_index"].numel()), what
                assert np.isin(case.expect, d4["exc_index"]).all() and n >= n_alt, what          # every large step is listed
                assert bool(s.flags & RERUN) == (n > cap0), (what, n, cap0, s.flags)
                assert_same_result(result_of(eng, s), want, what + ": decoded on the device")
                seen[n] = n_alt
            finally:
                eng.close()
    print(f"totals {min(seen)} .. {max(seen)} for {cap0 - 40} .. {cap0 + 2} alternating reads")
    assert cap0 in seen and cap0 + 1 in seen, (cap0, sorted(seen))


# ---- 3. the fetch contract as the ABI has it ------------------------------------------------------------------------------------------

def raw_fetch(eng, width, exc_cap, n_bins, room, give=("cov", "index", "value")):
    """raft_hip_fetch_packed_w / raft_hip_fetch_delta4 through ctypes: the code, *n_exc, and the arrays (filled with marks before)."""
    P = lambda a: C.c_void_p(a.ctypes.data)
    n = C.c_int64(-5)
    xi, xv = np.full(room, MARK, np.int64), np.full(room, MARK, np.int32)
    pi, pv = P(xi) if "index" in give else None, P(xv) if "value" in give else None
    if width == 8:
        cov, anchor = np.full((n_bins + 1) // 2 + 1, 0xA5, np.uint8), np.full((n_bins + 1023) // 1024 + 1, MARK, np.int32)
        rc = eng._lib.raft_hip_fetch_delta4(eng._ctx, None, P(cov) if "cov" in give else None, P(anchor) if "cov" in give else None, exc_cap, pi, pv,
                                            C.byref(n), *[None] * 7)
    else:
        cov, anchor = np.full(n_bins + 1, 0xA5A5 if width == 2 else 0xA5, np.uint16 if width == 2 else np.uint8), None
        rc = eng._lib.raft_hip_fetch_packed_w(eng._ctx, width, None, P(cov) if "cov" in give else None, exc_cap, pi, pv, C.byref(n), *[None] * 7)
    return rc, int(n.value), cov, anchor, xi, xv


def untouched(cov, anchor, xi, xv):
    return (cov == cov.dtype.type(0xA5A5 & np.iinfo(cov.dtype).max)).all() and (anchor is None or (anchor == MARK).all()) and (xi == MARK).all() and (xv == MARK).all()


@pytest.mark.parametrize("spec", SMALL + [(1, "short", EXC_CAP_FLOOR + 1, EXC_CAP_FLOOR + 1 + 4 * EXC_COLD_W), (2, "long", EXC_CAP_FLOOR + 1, EXC_CAP_FLOOR + 1 + 4 * EXC_COLD_W),
                                          (8, "steps", EXC_CAP_FLOOR + 1, EXC_CAP_FLOOR + 1 + 4 * EXC_COLD_W)], ids=exc_case_id)
@pytest.mark.parametrize("first", ["pass", "reencode"])
def test_fetch_contract(spec, first):
    """After a pass that lists n = 0, 1, 2 or cap0 + 1 windows (in the set's width, or in int32 and encoded by the fetch): the size query
    gives n; one entry short of room gives ERR_TOO_LARGE, n, and writes nothing; exactly n succeeds; n + 1 leaves entry n alone."""
    from raft_amd import engine
    case, want = built(spec)
    cov = want["cov"]
    width, B = case.width, case.B
    eng = engine.Engine(case.p, device=0)
    try:
        eng.set_output_width(4 if (first == "reencode" or width == 8) else width)
        eng.run_host(*case.query_cols())
        eng.finish()
        what = f"set {case.name}, first {first}"
        rc, n, *_ = raw_fetch(eng, width, 0, B, 1, give=())
        assert rc == engine.OK and n == case.K, (what, rc, n)                          # the size query
        rc, n, *_ = raw_fetch(eng, width, -1, B, 1, give=())
        assert rc == engine.OK and n == case.K, (what, rc, n)                          # ... whatever exc_cap says
        for give in (("cov",), ("index",), ("value",), ("cov", "index", "value")):
            rc, n, *arrays = raw_fetch(eng, width, case.K - 1, B, case.K + 2, give=give)
            assert rc == engine.ERR_TOO_LARGE and n == case.K and untouched(*arrays), (what, give, rc, n)
        for room in (case.K, case.K + 1):
            rc, n, codes, anchor, xi, xv = raw_fetch(eng, width, room, B, case.K + 2)
            assert rc == engine.OK and n == case.K, (what, room, rc, n)
            assert np.array_equal(xi[:n], case.expect) and np.array_equal(xv[:n], cov[case.expect]), (what, room)
            assert (xi[n:] == MARK).all() and (xv[n:] == MARK).all(), (what, room)     # entry n and what follows: as they were
            if width == 8:
                from raft_amd import hostio
                assert np.array_equal(hostio.unpack_coverage_d4(B, codes[:-1], anchor[:-1], xi[:n], xv[:n]), cov), (what, room)
                assert codes[(B + 1) // 2:].tolist() == [0xA5] * (codes.size - (B + 1) // 2) and anchor[-1] == MARK, (what, room)
            else:
                assert np.array_equal(decode(codes[:-1], xi[:n], xv[:n]), cov) and codes[-1] == codes.dtype.type(0xA5A5 & np.iinfo(codes.dtype).max), (what, room)
    finally:
        eng.close()


# ---- 4. the host pipelines at the caller's capacity ------------------------------------------------------------------------------------

PIPE_FORMS = ("columns", "grouped", "windows", "shuffled")


@functools.lru_cache(maxsize=3)
def pipeline_set(width):
    """make_overlaps(4000 reads, seed 81) -- a set the planner cuts (test_gpu_delta4) -- with three hot reads, the first, one in the middle and
    the last: 255 (width 2: 65,535) self overlaps over the whole read on top of what the read has.  Whatever the chunks, the first
    chunk's share of the list is one of the running totals behind a hot read."""
    from raft_amd import hostio
    from raft_amd.synth import make_overlaps
    o = make_overlaps(n_reads=4000, seed=81)
    cols = [c.numpy() for c in (o.read_len,) + o.columns()]
    rl = cols[0]
    hot = np.array([0, o.n_reads // 2, o.n_reads - 1], np.int32)
    depth = EXC_LIMIT[2 if width == 2 else 1]
    h = np.repeat(hot, depth)
    add = [h, np.zeros(h.size, np.int32), rl[h], h, np.zeros(h.size, np.int32), rl[h]]
    rec = [np.concatenate([c, a]) for c, a in zip(cols[1:], add)]
    order = np.argsort(rec[0], kind="stable")
    cols = [rl] + [np.ascontiguousarray(c[order]) for c in rec]
    p = RaftParams(est_cov=30)
    want = oracle_run(p, *cols)
    off = hostio.group_offsets(o.n_reads, cols[1])
    assert off is not None and off.shape[0] == 1
    win = hostio.pack_windows(cols[2], cols[3], p.reso)
    perm = np.random.default_rng(3).permutation(len(cols[1]))
    perm = np.concatenate([[0], perm[perm != 0]])                                   # (record 0 stays first: it decides the symmetric flag)
    shuffled = [c[perm] for c in cols[1:4]]
    for a in list(want.values()) + cols:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return RaftParams(**dict(p.__dict__, symmetric_mode=1)), cols, want, off, win, shuffled, hot


def pipelined(eng, data, form, n_chunks, out, others):
    p, cols, want, off, win, shuffled, hot = data
    if form == "columns":
        return eng.run_pipelined(cols[0], cols[1], cols[2], cols[3], n_chunks=n_chunks, out=out, others=others)
    if form == "shuffled":
        return eng.run_pipelined(cols[0], shuffled[0], shuffled[1], shuffled[2], n_chunks=n_chunks, out=out, others=others)
    if form == "grouped":
        return eng.run_pipelined_grouped(cols[0], off, cols[2], cols[3], n_chunks=n_chunks, out=out, others=others)
    return eng.run_pipelined_windows(cols[0], off, win, n_chunks=n_chunks, out=out, others=others)


def capped(full, cap):
    """The caller's arrays with the exception list cut to `cap` entries; the whole list is marked first."""
    full["exc_index"][:] = MARK; full["exc_value"][:] = MARK
    return dict(full, exc_index=full["exc_index"][:cap], exc_value=full["exc_value"][:cap])


def marks_behind(full, cap):
    return (full["exc_index"][cap:] == MARK).all() and (full["exc_value"][cap:] == MARK).all()


@pytest.mark.parametrize("n_ctx", [1, 2])
@pytest.mark.parametrize("form", PIPE_FORMS)
@pytest.mark.parametrize("width", [1, 2])
def test_pipelines_at_the_callers_capacity(width, form, n_ctx):
    """exc_cap = 0, every running total behind a hot read (a first chunk's share: that chunk fits, the next does not), E - 1: the call
    says RAFT_HIP_ERR_TOO_LARGE and E, whichever chunk finished first (twice each), and writes nothing behind exc_cap; E and E + 1:
    the list, ascending, is the closed form, and every other array the oracle's."""
    from raft_amd import engine
    data = pipeline_set(width)
    p, cols, want, off, win, shuffled, hot = data
    cov, cov_off = want["cov"], want["cov_offset"]
    limit = EXC_LIMIT[width]
    big = exc_closed_list(cov, width)
    E = int(big.size)
    shares = [int((big < cov_off[h + 1]).sum()) for h in hot]
    assert 0 < shares[0] < shares[1] < shares[2] == E, shares                        # (the base set itself lists nothing: the hot reads are the list)
    eng = engine.Engine(p, device=0)
    others = [engine.Engine(RaftParams(est_cov=3, reso=7, symmetric_mode=1), device=0) for _ in range(n_ctx - 1)]
    full = eng.host_output_buffers(cols[0], pinned=False, exc_cap=E + 8, width=width)
    try:
        for n_chunks in (1, 2, 3):
            for cap in (0, shares[0], shares[1], E - 1):
                for rep in range(2):
                    what = f"width {width}, form {form}, {n_ctx} contexts, {n_chunks} chunks, exc_cap {cap} of {E}, call {rep}"
                    with pytest.raises(engine.RaftError) as e:
                        pipelined(eng, data, form, n_chunks, capped(full, cap), others)
                    assert e.value.code == engine.ERR_TOO_LARGE and eng.last_n_exc == E, (what, e.value.code, eng.last_n_exc)
                    assert marks_behind(full, cap), what
            for cap in (E, E + 1):
                what = f"width {width}, form {form}, {n_ctx} contexts, {n_chunks} chunks, exc_cap {cap} of {E}"
                res, s = pipelined(eng, data, form, n_chunks, capped(full, cap), others)
                assert eng.last_n_exc == E and marks_behind(full, E), what
                if n_chunks >= 2:
                    assert s.n_devices_used == n_ctx, (what, s.n_devices_used)             # (the set was cut: every context had a chunk)
                assert np.array_equal(res["exc_index"], big) and np.array_equal(res["exc_value"], cov[big]), what
                assert res["cov8"].dtype == (np.uint8 if width == 1 else np.uint16) and np.array_equal(res["cov8"], np.minimum(cov, limit)), what
                for k in ("cov_offset", "rep_offset", "rep_s", "rep_e", "frag_offset", "frag_begin", "frag_end"):
                    assert np.array_equal(res[k], want[k]), (what, k)
                assert (s.symmetric, s.high_cov, s.total_coverage, s.total_windows, s.total_repeat_length, s.total_read_length) == \
                    tuple(want[k] for k in ("symmetric", "high_cov", "total_coverage", "total_windows", "total_repeat_length", "total_read_length")), what
    finally:
        for e2 in [eng] + others:
            e2.close()


@pytest.mark.parametrize("n_ctx", [1, 2])
@pytest.mark.parametrize("form", PIPE_FORMS)
def test_pipelines_four_bit_steps_at_the_reported_capacity(form, n_ctx):
    """Four-bit steps: the total E -- the large steps and the first windows of the tiles of every chunk -- is no closed form, so the
    contract itself is the test: without room the call reports an E that is at least the number of large steps; with exactly E it
    succeeds and decodes to the oracle's array; with E - 1 it fails again, reporting the same E."""
    from raft_amd import engine
    data = pipeline_set(8)
    p, cols, want, off, win, shuffled, hot = data
    steps = int(exc_closed_list(want["cov"], 8).size)
    eng = engine.Engine(p, device=0)
    others = [engine.Engine(RaftParams(est_cov=3, reso=7, symmetric_mode=1), device=0) for _ in range(n_ctx - 1)]
    full = eng.host_output_buffers(cols[0], pinned=False, exc_cap=4 * steps + 65536, width=8)
    try:
        for n_chunks in (1, 2, 3):
            what = f"form {form}, {n_ctx} contexts, {n_chunks} chunks"
            with pytest.raises(engine.RaftError) as e:
                pipelined(eng, data, form, n_chunks, capped(full, 0), others)
            E = eng.last_n_exc
            assert e.value.code == engine.ERR_TOO_LARGE and steps <= E <= full["exc_index"].size and marks_behind(full, 0), (what, E, steps)
            res, s = pipelined(eng, data, form, n_chunks, capped(full, E), others)
            assert eng.last_n_exc == E and res["exc_index"].size == E and marks_behind(full, E), (what, eng.last_n_exc, E)
            check_pipelined_d4(res, s, want, what)
            assert np.isin(exc_closed_list(want["cov"], 8), res["exc_index"]).all(), what
            for rep in range(2):
                with pytest.raises(engine.RaftError) as e:
                    pipelined(eng, data, form, n_chunks, capped(full, E - 1), others)
                assert e.value.code == engine.ERR_TOO_LARGE and eng.last_n_exc == E and marks_behind(full, E - 1), (what, rep, eng.last_n_exc, E)
    finally:
        for e2 in [eng] + others:
            e2.close()


def test_pipeline_into_page_locked_arrays_of_exactly_the_size():
    from raft_amd import engine
    data = pipeline_set(1)
    p, cols, want, off, win, shuffled, hot = data
    big = exc_closed_list(want["cov"], 1)
    eng = engine.Engine(p, device=0)
    other = engine.Engine(p, device=0)
    try:
        out = eng.host_output_buffers(cols[0], pinned=True, exc_cap=int(big.size), width=1)
        assert out["exc_index"].size == big.size
        for form in PIPE_FORMS:
            for others in ([], [other]):
                out["exc_index"][:] = MARK; out["exc_value"][:] = MARK
                res, s = pipelined(eng, data, form, 3, out, others)
                assert np.array_equal(res["exc_index"], big) and np.array_equal(res["exc_value"], want["cov"][big]), (form, len(others))
                assert np.array_equal(decode(res["cov8"], res["exc_index"], res["exc_value"]), want["cov"]), (form, len(others))
    finally:
        eng.close(); other.close()
