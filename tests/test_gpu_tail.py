"""GPU: the per-read tail of a pass (raft_amd/csrc/finalize.hpp: finalize_count_kernel -> tail_prefix_kernel -> finalize_fill_kernel<CUTS>
/ finalize_cuts_kernel) at every structural boundary -- the tail sets of raft_testlib; what they hold and that they hold it:
tests/test_tail_cases.py.

Every set and parameter triple (div, overlap, flank) goes through Engine.run_host + finish + fetch, bit-exact against the oracle:
with the cut points written by the fill kernel and by finalize_cuts_kernel on the first fetch (set_emit_cuts), through both pileup
kernels (the deep kernel emits the raw runs in code of its own), twice on one context (the second pass is the speculative one, and
finalize_count_kernel sorts the raw arrays in place), once through the general bucketing, and through the host pipeline in one and
three chunks (repeats, fragments and offsets: its outputs hold no cut points).  tail_offsets compares the FULL offset arrays and the
totals on either side of 262,144 reads, what one workgroup of tail_prefix_kernel scans.  A failure names the set, the triple, the
variation and the first differing read with its length, repeats, lane, wave and workgroup.  RAFT_HIP_ERR_FRAGMENT must name the
FIRST read that cannot be split, among several in different waves and workgroups.
"""
import numpy as np
import pytest
from raft_testlib import (KERNELS, TAIL_COUNTS_FLANKS, TAIL_COUNTS_L, TAIL_DIVS, TAIL_ERROR_READS, TAIL_FLANKS, TAIL_MARKERS_L, TAIL_NS,
                          TAIL_PIECES_TRIPLES, OracleError, RaftParams, assert_matches_ref_fuzz, assert_tail_result, kernel_mode, tail_counts,
                          tail_error_set, tail_first_difference, tail_markers, tail_offsets, tail_overlaps, tail_pieces, tail_ref_case, tail_ref_count)
from test_gpu_delta4 import result_of

pytestmark = pytest.mark.gpu

SCALARS = ("symmetric", "high_cov", "total_coverage", "total_windows", "total_repeat_length", "total_read_length")


def check_counts(s, want, what):
    assert (s.n_reads, s.n_repeats, s.n_cuts, s.n_fragments) == (want["n_reads"], want["rep_s"].size, want["cuts"].size, want["frag_read"].size), \
        (what, s.n_reads, s.n_repeats, s.n_cuts, s.n_fragments)


def one_pass(eng, case, want, what):
    eng.run_host(*case.query_cols())
    s = eng.finish()
    assert_tail_result(case, result_of(eng, s), want, what)
    check_counts(s, want, what)


def pipelined(eng, case, want, what):
    """The host pipeline in one and three chunks: repeats, fragments, offsets (the jobs' offsets are concatenated) and the totals."""
    from raft_amd import hostio
    rl, qid, qs, qe = case.cols[:4]
    for n_chunks in (1, 3):
        w = f"{what}, host pipeline in {n_chunks} chunks"
        res, s = eng.run_pipelined(rl, qid, qs, qe, n_chunks=n_chunks)
        msg = tail_first_difference(case, {k: res[k] for k in ("rep_offset", "rep_s", "rep_e", "frag_offset", "frag_begin", "frag_end")}, want)
        assert msg is None, f"{w}: {msg}"
        assert np.array_equal(hostio.unpack_coverage(res["cov8"], res["exc_index"], res["exc_value"]), want["cov"]), w
        assert tuple(getattr(s, k) for k in SCALARS) == tuple(want[k] for k in SCALARS), (w, [(k, getattr(s, k), want[k]) for k in SCALARS])
        assert s.n_fragments == want["frag_read"].size and s.n_repeats == want["rep_s"].size, w


def through_the_tail(eng, case, want, with_pipeline=True):
    """Every variation of the module's docstring on one context that holds the case's parameters."""
    for kernel in KERNELS:
        with kernel_mode(kernel):
            for cuts in (True, False):
                eng.set_emit_cuts(cuts)
                for it in (1, 2):
                    one_pass(eng, case, want, f"{kernel} kernel, cut points by the {'fill kernel' if cuts else 'first fetch'}, pass {it}")
    eng.set_emit_cuts(True)
    eng.set_tuning(0, True, -1)
    try:
        one_pass(eng, case, want, "general bucketing")
    finally:
        eng.set_tuning(0, False, -1)
    if with_pipeline:
        pipelined(eng, case, want, "wave kernel")


def engine_for(p):
    from raft_amd import engine
    return engine.Engine(p, device=0)


@pytest.mark.parametrize("div", TAIL_DIVS)
def test_markers(div):
    eng = None
    try:
        for flank in TAIL_FLANKS:
            for overlap in tail_overlaps(div, TAIL_MARKERS_L):
                case = tail_markers(div, overlap, flank)
                if eng is None:
                    eng = engine_for(case.p)
                else:
                    eng.set_params(case.p)             # one context, reused under every triple
                through_the_tail(eng, case, case.oracle())
    finally:
        if eng is not None:
            eng.close()


@pytest.mark.parametrize("flank", TAIL_COUNTS_FLANKS)
@pytest.mark.parametrize("div", (1, 3))
def test_counts(div, flank):
    eng = None
    try:
        for overlap in (0, TAIL_COUNTS_L):
            case = tail_counts(div, overlap, flank)
            if eng is None:
                eng = engine_for(case.p)
            else:
                eng.set_params(case.p)
            through_the_tail(eng, case, case.oracle())
    finally:
        if eng is not None:
            eng.close()


@pytest.mark.parametrize("triple", TAIL_PIECES_TRIPLES)
def test_pieces(triple):
    case = tail_pieces(*triple)
    eng = engine_for(case.p)
    try:
        through_the_tail(eng, case, case.oracle())
    finally:
        eng.close()


def test_offsets_up_to_a_workgroup_and_a_read():
    eng = None
    try:
        for N in (n for n in TAIL_NS if n <= 257):
            case = tail_offsets(N)
            if eng is None:
                eng = engine_for(case.p)
            through_the_tail(eng, case, case.oracle(), with_pipeline=N > 0)
    finally:
        if eng is not None:
            eng.close()


@pytest.mark.parametrize("N", [n for n in TAIL_NS if n > 257])
def test_offsets_around_a_workgroup_of_the_prefix_kernel(N):
    """The FULL rep_offset, cut_offset, frag_offset arrays, the totals and the summary's counts; the wave kernel, one pass per
    setting of emit_cuts."""
    case = tail_offsets(N)
    want = case.oracle()
    eng = engine_for(case.p)
    try:
        for cuts in (True, False):
            eng.set_emit_cuts(cuts)
            one_pass(eng, case, want, f"wave kernel, cut points by the {'fill kernel' if cuts else 'first fetch'}")
    finally:
        eng.close()


def test_fragment_error_names_the_first_read():
    """overlap = div*L + 1: reads 3, 70, 300 and 700 -- waves and workgroups apart -- would begin their second fragment at -1, every
    other read stays whole.  The engine raises ERR_FRAGMENT for read 3, the smallest index; with read 3 made short, for read 70; the
    same context then runs a tail_markers set under a legal triple."""
    from raft_amd import engine
    eng = None
    try:
        for short, first in (((), TAIL_ERROR_READS[0]), (TAIL_ERROR_READS[:1], TAIL_ERROR_READS[1])):
            case = tail_error_set(short)
            assert case.expect["error_read"] == first
            with pytest.raises(OracleError) as oe:
                case.oracle()
            assert oe.value.code == engine.ERR_FRAGMENT
            if eng is None:
                eng = engine_for(case.p)
            for cuts in (True, False):
                eng.set_emit_cuts(cuts)
                with pytest.raises(engine.RaftError) as ge:
                    eng.run_host(*case.query_cols())
                    eng.finish()
                assert ge.value.code == engine.ERR_FRAGMENT and ge.value.index == first, (short, cuts, ge.value.code, ge.value.index)
        eng.set_emit_cuts(True)
        legal = tail_markers(2, 1, 2)
        eng.set_params(legal.p)
        one_pass(eng, legal, legal.oracle(), "after two failed passes on the context")
    finally:
        if eng is not None:
            eng.close()


def test_engine_equals_the_reference_binary_on_the_tail_sets():
    """tests/golden/tail_ref.npz: the sets as the unmodified reference binary answered them (repeat_length = interval_length)."""
    eng = None
    try:
        for i in range(tail_ref_count()):
            name, case, exp = tail_ref_case(i)
            p = RaftParams(**dict(case.p.__dict__, symmetric_mode=-1))
            if eng is None:
                eng = engine_for(p)
            else:
                eng.set_params(p)
            eng.run_host(*case.cols)
            s = eng.finish()
            what = f"tail_ref case {i} ({name}, {case.triple})"
            got = result_of(eng, s)
            msg = tail_first_difference(case, {k: v for k, v in got.items() if not k.startswith("cut")}, dict(exp, frag_offset=got["frag_offset"]))
            assert msg is None, f"{what}: {msg}"
            assert_matches_ref_fuzz(got, exp, p, what)
    finally:
        if eng is not None:
            eng.close()
