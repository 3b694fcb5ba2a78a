"""GPU: both pileup kernels at every structural boundary and value threshold (the lattice sets of raft_testlib; what they hold and
that they hold it: tests/test_lattice_cases.py).

The random sets of the other suites place runs of high windows anywhere; these place ONE run per read so that it ends on the last
slot of a lane / half-row / row / tile / piece and begins on the first slot after it, at every alignment of the read's offset, one
window short of repeat_length and exactly long enough -- the cases the packed prefix, the DPP scan over both half-rows, the carry
along the rows and the piece-edge rule of finalize_count_kernel must all get right -- and put values on either side of every
threshold in the code: high_cov - 1 next to high_cov, high_cov = 1 / 32767 / 32768 / 65537, coverage 254 / 255 / 256 and
65534 ... 65537 (the encodings' escapes), steps of 7 and 8 (the four-bit codes), tiles of 32767 and 32768 intervals (the hand-over to
pileup_deep_kernel).  Every set goes through both kernels (raft_testlib.KERNELS), every input form (coordinate columns, grouped,
window records, the general bucketing), every encoding (int32, one / two bytes, four-bit steps, with the checkers of
test_gpu_packed_output / test_gpu_delta4) and, for the column form, ranges that begin elsewhere (set_tuning tile_bins).
Bit-exact against the oracle; a failure names set, form, kernel, width and the first differing read as (a, d, W, offset mod 4).
"""
import numpy as np
import pytest
from raft_testlib import (DEPTH_NS, KERNELS, assert_lattice_result, kernel_mode, lattice_byte_level, lattice_depth, lattice_first_difference,
                          lattice_pieces, lattice_rows, lattice_steps, lattice_tile_end)
from test_gpu_deep import DEEP, RERUN
from test_gpu_delta4 import all_forms, result_of
from test_gpu_packed_output import check_against, run_width

pytestmark = pytest.mark.gpu

FORMS = ("columns", "grouped", "windows", "bucket")


def runner(eng, case, form):
    """-> run(): one pass over the set in the given input form, finished."""
    from raft_amd import hostio
    rl, qid, qs, qe = case.cols[:4]
    if form in ("columns", "bucket"):
        def run():
            eng.run_host(rl, qid, qs, qe, None, None, None)
            return eng.finish()
        return run
    off = hostio.group_offsets(case.n_reads, qid)
    assert off is not None and off.shape[0] == 1
    if form == "grouped":
        def run():
            eng.run_host_grouped(rl, off, qs, qe)
            return eng.finish()
        return run
    win = hostio.pack_windows(qs, qe, case.p.reso)
    assert win is not None

    def run():
        eng.run_host_windows(rl, off, win)
        return eng.finish()
    return run


def located(case, want, what, eng, check):
    """Runs a checker of another suite; when it fails, the message gains the set, `what` and the lattice coordinate of the first
    read whose int32 arrays (the last pass's, as the device decodes them) differ."""
    try:
        return check()
    except AssertionError as e:
        try:
            where = lattice_first_difference(case, eng.fetch(), want) if eng is not None else None
        except Exception as e2:                                       # (the fetch itself may be what fails)
            where = f"fetch failed: {e2}"
        raise AssertionError(f"set {case.name}, {what}: {where or 'the int32 arrays agree: the fault is in the encoding or its lists'}\n{e}") from e


def check_width2_lists(eng, want, what):
    """The two-byte encoding lists exactly the windows at or above 65,535, ascending, with their true values."""
    f = eng.fetch_packed(width=2)
    big = np.flatnonzero(want["cov"] >= 65535)
    assert f["cov8"].dtype == np.uint16 and np.array_equal(f["cov8"], np.minimum(want["cov"], 65535).astype(np.uint16)), what
    assert np.array_equal(f["exc_index"], big), (what, f["exc_index"][:8], big[:8])
    assert np.array_equal(f["exc_value"], want["cov"][big]), (what, f["exc_value"][:8], want["cov"][big][:8])


def through_everything(case, want):
    from raft_amd import engine
    for kernel in KERNELS:
        with kernel_mode(kernel):
            # four-bit steps made from an int32 pass and written by the pass; int32 decoded on the device after every width
            for form, tile_bins in (("columns", 0), ("columns", 512), ("columns", 1000), ("grouped", 0), ("windows", 0), ("bucket", 0)):
                what = f"form {form}, tile_bins {tile_bins}, kernel {kernel}"
                eng = engine.Engine(case.p, device=0)
                try:
                    eng.set_tuning(tile_bins, form == "bucket", -1)
                    run = runner(eng, case, form)
                    eng.set_output_width(4)
                    assert_lattice_result(case, result_of(eng, run()), want, what + ", width 4")
                    located(case, want, what + ", widths 4 / 8 / 1 / 8 (all_forms)", eng, lambda: all_forms(eng, run, want, f"{case.name}: {what}"))
                    eng.set_output_width(2)
                    s = run()
                    pk = eng.packed_device()
                    assert pk is not None and pk["width"] == 2, what
                    assert_lattice_result(case, result_of(eng, s), want, what + ", width 2")
                    located(case, want, what + ", width 2 lists", eng, lambda: check_width2_lists(eng, want, what))
                finally:
                    eng.close()
        # one and two bytes per window as the pass wrote them: codes, listed windows ascending, their values
        for bucket in (False, True):
            for width in (1, 2):
                what = f"form {'bucket' if bucket else 'columns'}, kernel {kernel}, width {width}"
                res = run_width(case.p, case.query_cols(), width, variant=kernel, force_bucket=bucket)
                assert res["packed"] is not None, what
                assert_lattice_result(case, res["fetch"], want, what)
                located(case, want, what + " (check_against)", None, lambda: check_against(res, want, width, f"{case.name}: {what}"))


@pytest.mark.parametrize("which", ["r50", "r7", "flank", "h1"])
def test_rows_and_threshold(which):
    case = lattice_rows(which)
    through_everything(case, case.oracle())


def test_tile_end():
    case = lattice_tile_end()
    through_everything(case, case.oracle())


def test_pieces():
    case = lattice_pieces()
    through_everything(case, case.oracle())


def test_byte_level():
    case = lattice_byte_level()
    want = case.oracle()
    assert int((want["cov"] >= 255).sum()) > 4096          # (more escaped windows than the list's first size holds)
    through_everything(case, want)


def test_steps():
    case = lattice_steps()
    through_everything(case, case.oracle())


@pytest.mark.parametrize("H", [3, 32767, 32768, 65537])
def test_depth(H):
    case = lattice_depth(H)
    want = case.oracle()
    assert want["cov"].max() == 65537 and int((want["cov"] >= 65535).sum()) >= 3
    through_everything(case, want)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("H", [3, 32767, 32768, 65537])
def test_depth_which_kernel_took_the_tile(H, form, monkeypatch):
    """summary.flags: with every read alone in its tile, a read's record count is the tile's.  32,767 intervals on one window are
    piled up by the wave kernel itself (no tile listed for the deep kernel, nothing run again); from 32,768 the deep kernel takes
    the tile, in the same pass.  A second pass on the context (the speculative one) does the same."""
    from raft_amd import engine
    monkeypatch.delenv("RAFT_DEEP_MIN", raising=False)      # (a process that lowers the threshold lists every tile: here it stays at 2^15)
    for Ns in (tuple(n for n in DEPTH_NS if n <= 32767), DEPTH_NS):
        case = lattice_depth(H, Ns)
        want = case.oracle()
        assert want["cov"].max() == max(Ns)
        what = f"form {form}, kernel wave, N up to {max(Ns)}"
        for width in (4, 2):                                 # (a context per width: nothing but the data decides what its passes do)
            eng = engine.Engine(case.p, device=0)
            try:
                eng.set_tuning(0, form == "bucket", -1)
                run = runner(eng, case, form)
                eng.set_output_width(width)
                for it in range(2):
                    s = run()
                    assert_lattice_result(case, result_of(eng, s), want, f"{what}, width {width}, pass {it}")
                    if max(Ns) <= 32767:
                        assert not (s.flags & DEEP) and not (s.flags & RERUN), (what, width, it, s.flags)
                    else:
                        assert s.flags & DEEP and not (s.flags & RERUN), (what, width, it, s.flags)
                    if width == 2:
                        located(case, want, f"{what}, width 2 lists, pass {it}", eng, lambda: check_width2_lists(eng, want, what))
            finally:
                eng.close()
