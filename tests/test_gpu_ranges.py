"""GPU: the pileup's range boundaries -- the graded quantum and the hand-out's shares -- on the sets of tests/range_cases.py (what they
hold and that they hold it: tests/test_range_cases.py; the boundaries themselves against raft_amd/csrc/quantum.hpp: tests/test_quantum.py).

pileup_wave_kernel's workers draw ranges of reads from hand-out counters; where a range may begin is the pass's quantum.  The engine
grades it only from 1,072,693,248 windows on, so every graded set here runs under RAFT_GRADED_MIN=0 and every test asserts
SUM_GRADED_RANGES: the route a case claims is the route that ran.  The sets put reads, reads of one and of no window, read ends and
runs of high windows on at(k) - 1, at(k), at(k) + 1 for every kind of boundary (first of a share, long to long, long to short, short
to short, the short closing range, the set's last), leave ranges and shares without a read, and go through every input form
(columns as one and as three sorted runs, grouped with and without the window count, window records, the general bucketing), both
kernels, every output width, the three forms of a pass on one context, the host pipeline, and changes of the quantum between passes
over the same tensors (no pass under a new quantum may be built on the last one's boundaries).  The uniform sets put the same
placements at the first and last range of every counter's share for n_ranges below 8, not a multiple of 8, around the worker count
and at several draws per worker.  Bit-exact against the oracle; a failure names the set, the variation, the first differing read,
its boundary class and k.

Not here: more ranges than workers under the GRADED quantum begins near 10^8 windows; that regime stays with tools/full_compare.py
and bench.py --full.  The uniform sets cover the same hand-out arithmetic (several draws per worker) at 10^6 to 10^7 windows.

Measured on an MI355X: the module's 54 tests take 4.4 s; the slowest is the first to run, test_graded_every_form[100-wave], with
1.8 s (the process's first context), behind it test_graded_every_width[7200000] with 0.35 s.
"""
import numpy as np
import pytest
import range_cases as R
from raft_testlib import KERNELS, assert_lattice_result, kernel_mode
from test_gpu_configs import check_pipelined
from test_gpu_delta4 import all_forms, result_of
from test_gpu_lattice import check_width2_lists, located

pytestmark = pytest.mark.gpu

FORMS = ("columns", "three runs", "grouped, window count", "grouped, window count, no fused head", "grouped", "windows, window count", "windows", "bucket")


def flags_of(s):
    from raft_amd import engine
    names = {"graded": engine.SUM_GRADED_RANGES, "speculated": engine.SUM_SPECULATED, "kept": engine.SUM_KEPT_GEOMETRY, "rerun": engine.SUM_RERUN}
    return {k for k, v in names.items() if s.flags & v}


def runner(eng, case, form, monkeypatch):
    """-> run(): one pass over the set in the given input form, finished."""
    from raft_amd import hostio
    rl, qid, qs, qe = case.cols[:4]
    if form in ("columns", "bucket"):
        def run():
            eng.run_host(rl, qid, qs, qe, None, None, None)
            return eng.finish()
        return run
    if form == "three runs":
        q3, s3, e3 = R.three_runs(case)
        big = q3.size > 100                      # (the sets of a handful of records do not fill three runs)
        assert np.flatnonzero(np.diff(q3) < 0).size == 2 or not big

        def run():
            eng.run_host(rl, q3, s3, e3, None, None, None)
            s = eng.finish()
            assert s.interval_path == 0 and (s.n_segments == 3 or not big), (case.name, form, s.n_segments)
            return s
        return run
    off = hostio.group_offsets(case.n_reads, qid)
    assert off is not None and off.shape[0] == 1
    n_bins = case.B if "window count" in form else -1
    if form.startswith("grouped"):
        def run():
            if "no fused head" in form:
                monkeypatch.setenv("RAFT_NO_FUSED_HEAD", "1")
            try:
                eng.run_host_grouped(rl, off, qs, qe, n_bins=n_bins)
                return eng.finish()
            finally:
                monkeypatch.delenv("RAFT_NO_FUSED_HEAD", raising=False)
        return run
    win = hostio.pack_windows(qs, qe, case.p.reso)
    assert win is not None

    def run():
        eng.run_host_windows(rl, off, win, n_bins=n_bins)
        return eng.finish()
    return run


def check(case, eng, s, want, what, graded, rerun_ok=False):
    """rerun_ok: with every tile sent the deep kernel's way a set of more than 1024 tiles outgrows the list of deep tiles, and
    raft_hip_finish runs the pass again with room -- under the same quantum, which the flag of the pass that produced the results says."""
    assert ("graded" in flags_of(s)) == graded, f"set {case.name}, {what}: flags {sorted(flags_of(s))}"
    assert rerun_ok or "rerun" not in flags_of(s), f"set {case.name}, {what}: flags {sorted(flags_of(s))}"
    assert_lattice_result(case, result_of(eng, s), want, what)


@pytest.fixture(scope="module")
def wanted():
    """The oracle's result per set, computed once and left unchanged."""
    cache = {}

    def get(case):
        if case.name not in cache:
            cache[case.name] = case.oracle()
            for v in cache[case.name].values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        return cache[case.name]
    return get


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("B", R.GRADED_BS)
def test_graded_every_form(B, kernel, wanted, monkeypatch):
    from raft_amd import engine
    case = R.ranges_graded(B)
    want = wanted(case)
    monkeypatch.setenv("RAFT_GRADED_MIN", "0")
    with kernel_mode(kernel):
        for form in FORMS:
            eng = engine.Engine(case.p, device=0)
            try:
                eng.set_tuning(0, form == "bucket", -1)
                s = runner(eng, case, form, monkeypatch)()
                check(case, eng, s, want, f"form {form}, kernel {kernel}, width 4", True, rerun_ok=kernel == "deep" and B > 1024 * R.TILE_CAP)
                assert s.interval_path == int(form == "bucket"), (case.name, form)
            finally:
                eng.close()


@pytest.mark.parametrize("B", R.GRADED_BS)
def test_graded_every_width(B, wanted, monkeypatch):
    """Widths 4, 8, 1, 8 (all_forms) and 2 on the columns form: with the four-bit steps the tiles' slots and ids come from
    n_tiles = 8 * per_share."""
    from raft_amd import engine
    case = R.ranges_graded(B)
    want = wanted(case)
    monkeypatch.setenv("RAFT_GRADED_MIN", "0")
    eng = engine.Engine(case.p, device=0)
    try:
        run = runner(eng, case, "columns", monkeypatch)
        what = "form columns, kernel wave"
        located(case, want, what + ", widths 4 / 8 / 1 / 8 (all_forms)", eng, lambda: all_forms(eng, run, want, f"{case.name}: {what}"))
        for width in (8, 1, 2, 4):
            eng.set_output_width(width)
            s = run()
            check(case, eng, s, want, f"{what}, width {width}", True)
            if width == 2:
                located(case, want, what + ", width 2 lists", eng, lambda: check_width2_lists(eng, want, what))
    finally:
        eng.close()


def test_four_bit_steps_when_tiles_have_no_slots_of_their_own(wanted, monkeypatch):
    from raft_amd import engine
    case = R.ranges_graded(888_833)
    want = wanted(case)
    monkeypatch.setenv("RAFT_GRADED_MIN", "0")
    monkeypatch.setenv("RAFT_EXTRA_CAP", "1")
    eng = engine.Engine(case.p, device=0)
    try:
        eng.set_output_width(8)
        s = runner(eng, case, "columns", monkeypatch)()
        check(case, eng, s, want, "form columns, kernel wave, width 8, RAFT_EXTRA_CAP=1", True)
    finally:
        eng.close()


def device_columns(case, cols=None):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0") for x in (cols or case.cols[:4])]


@pytest.mark.parametrize("three", [False, True], ids=["one run", "three runs"])
@pytest.mark.parametrize("B", R.GRADED_BS)
def test_graded_three_passes_on_one_context(B, three, wanted, monkeypatch):
    """From device tensors: the long way (tile_first_kernel), speculated with the geometry scanned again (PrepPost), speculated on
    kept geometry (the boundaries PrepPost wrote)."""
    from raft_amd import engine
    case = R.ranges_graded(B)
    want = wanted(case)
    monkeypatch.setenv("RAFT_GRADED_MIN", "0")
    dev = device_columns(case, (case.cols[0],) + R.three_runs(case) if three else None)
    eng = engine.Engine(case.p, device=0)
    try:
        for it, (scan_again, flags) in enumerate(((False, {"graded"}), (True, {"graded", "speculated"}), (False, {"graded", "speculated", "kept"}),
                                                  (False, {"graded", "speculated", "kept"}))):
            if scan_again:
                monkeypatch.setenv("RAFT_NO_KEEP_GEOMETRY", "1")
            eng.run_device(*dev)
            s = eng.finish()
            monkeypatch.delenv("RAFT_NO_KEEP_GEOMETRY", raising=False)
            what = f"device columns ({'three runs' if three else 'one run'}), pass {it}"
            if case.cols[1].size > 1:            # (a stream of one record is never verified in its kernels: nothing to speculate on)
                assert flags_of(s) == flags, f"set {case.name}, {what}: flags {sorted(flags_of(s))}, want {sorted(flags)}"
            check(case, eng, s, want, what, True)
    finally:
        eng.close()


def test_quantum_changes_between_passes_on_one_context(wanted, monkeypatch):
    """Graded, RAFT_GRADED_QUANTUM=0, graded, set_tuning(512), back -- over the same tensors.  The first pass under a quantum goes
    the long way (its boundaries are its own: neither speculated nor on kept geometry), the second keeps that pass's geometry; the
    flag follows the quantum."""
    from raft_amd import engine
    case = R.ranges_graded(888_833)
    want = wanted(case)
    dev = device_columns(case)
    eng = engine.Engine(case.p, device=0)

    def two_passes(what, graded):
        for it in range(2):
            eng.run_device(*dev)
            s = eng.finish()
            want_flags = ({"graded"} if graded else set()) | ({"speculated", "kept"} if it else set())
            assert flags_of(s) == want_flags, f"set {case.name}, {what}, pass {it}: flags {sorted(flags_of(s))}, want {sorted(want_flags)}"
            check(case, eng, s, want, f"{what}, pass {it}", graded)
    try:
        monkeypatch.setenv("RAFT_GRADED_MIN", "0")
        two_passes("graded", True)
        monkeypatch.setenv("RAFT_GRADED_QUANTUM", "0")
        two_passes("RAFT_GRADED_QUANTUM=0", False)
        monkeypatch.delenv("RAFT_GRADED_QUANTUM")
        two_passes("graded again", True)
        eng.set_tuning(512, False, -1)
        two_passes("set_tuning(512)", False)
        eng.set_tuning(0, False, -1)
        two_passes("graded once more", True)
        monkeypatch.delenv("RAFT_GRADED_MIN")
        two_passes("nothing set", False)
    finally:
        eng.close()


@pytest.mark.parametrize("B", [200_000, 888_832, 888_833])
def test_thresholds(B, wanted, monkeypatch):
    """RAFT_GRADED_MIN = n: uniform with B / kTileCap == n - 1, graded with B / kTileCap == n; nothing set: a small set is not graded."""
    from raft_amd import engine
    case = R.ranges_graded(B)
    want = wanted(case)
    tiles = B // R.TILE_CAP
    for setting, graded in ((None, False), (str(tiles + 1), False), (str(tiles), True), ("0", True), (str(R.GRADED_MIN_DEFAULT), False)):
        if setting is None:
            monkeypatch.delenv("RAFT_GRADED_MIN", raising=False)
        else:
            monkeypatch.setenv("RAFT_GRADED_MIN", setting)
        for form in ("columns", "grouped, window count"):
            eng = engine.Engine(case.p, device=0)
            try:
                s = runner(eng, case, form, monkeypatch)()
                check(case, eng, s, want, f"form {form}, RAFT_GRADED_MIN={setting}, B / kTileCap = {tiles}", graded)
            finally:
                eng.close()


@pytest.mark.parametrize("n_chunks", [1, 3])
def test_host_pipeline(n_chunks, wanted, monkeypatch):
    """run_pipelined: a chunk is a pass with a B of its own, graded by its own window count."""
    from raft_amd import engine
    case = R.ranges_graded(888_833)
    want = wanted(case)
    monkeypatch.setenv("RAFT_GRADED_MIN", "0")
    eng = engine.Engine(case.p, device=0)
    try:
        res, s = eng.run_pipelined(*case.cols[:4], n_chunks=n_chunks)
        what = f"set {case.name}, run_pipelined in {n_chunks} chunk(s)"
        assert s.flags & engine.SUM_GRADED_RANGES, what
        from raft_amd import hostio
        bad = np.flatnonzero(hostio.unpack_coverage(res["cov8"], res["exc_index"], res["exc_value"]) != want["cov"])
        if bad.size:
            r = int(np.searchsorted(want["cov_offset"], bad[0], side="right") - 1)
            raise AssertionError(f"{what}: cov differs in {bad.size} windows, first in {case.coordinate(r)}")
        check_pipelined(res, s, want, what)
        monkeypatch.delenv("RAFT_GRADED_MIN")
        res, s = eng.run_pipelined(*case.cols[:4], n_chunks=n_chunks)
        assert not s.flags & engine.SUM_GRADED_RANGES, what
        check_pipelined(res, s, want, what + ", nothing set")
    finally:
        eng.close()


@pytest.mark.parametrize("n_ranges", R.UNIFORM_NS)
def test_uniform_shares(n_ranges, wanted, monkeypatch):
    """set_tuning(256): columns and grouped, wave kernel, widths 4 and 1, two passes each."""
    from raft_amd import engine
    case = R.ranges_uniform(n_ranges)
    want = wanted(case)
    monkeypatch.delenv("RAFT_GRADED_MIN", raising=False)
    for form in ("columns", "grouped, window count", "grouped"):
        for width in (4, 1):
            eng = engine.Engine(case.p, device=0)
            try:
                eng.set_tuning(R.UNIFORM_Q, False, -1)
                eng.set_output_width(width)
                run = runner(eng, case, form, monkeypatch)
                for it in range(2):
                    check(case, eng, run(), want, f"form {form}, tile_bins 256 ({n_ranges} ranges), kernel wave, width {width}, pass {it}", False)
            finally:
                eng.close()


def test_graded_results_do_not_depend_on_who_draws_what(wanted, monkeypatch):
    """Five fresh contexts over the largest set with its share boundaries on short ranges: which worker helps which counter differs
    from run to run, the outputs must not -- bit-identical, and the oracle's."""
    from raft_amd import engine
    case = R.ranges_graded(5_900_000)
    want = wanted(case)
    monkeypatch.setenv("RAFT_GRADED_MIN", "0")
    first = None
    for it in range(5):
        eng = engine.Engine(case.p, device=0)
        try:
            s = runner(eng, case, "columns", monkeypatch)()
            assert "graded" in flags_of(s)
            got = result_of(eng, s)
        finally:
            eng.close()
        if first is None:
            first = got
            assert_lattice_result(case, got, want, "form columns, kernel wave, width 4, context 0")
        else:
            for k, v in first.items():
                same = np.array_equal(v, got[k]) if isinstance(v, np.ndarray) else v == got[k]
                assert same, f"set {case.name}, context {it}: {k} differs from context 0's"
