"""GPU: the buffers the queries beside the engine share on a context (raft_amd/csrc/engine_ctx.hpp q_len, q_col, q_csr_a, q_csr_b: the
staging of a host form; q_cov, q_abs: the coverage decoded to int32).  One context answers different queries one after the other, a
small input behind a large one, NULL columns behind a call that staged all six, a table with more runs behind one with fewer; and
low_coverage and repeat_stats decode the same pass into the same pair, across passes of different window counts.  Every answer is the
numpy model's (tests/test_*_cases.py) and, for the staging, the same call's on a fresh context."""
import numpy as np
import pytest
import test_fragment_overlaps_cases as frag_cases
import test_repeat_overlaps_cases as ovl_cases
import test_repeat_stats_cases as rst_cases
from raft_testlib import oracle_run
from test_gpu_repeat_stats import RESO, WIDTHS, window_runs, window_set
from test_low_cov_cases import same_low, want_low
from test_read_stats_cases import overlaps_for

from raft_amd.params import RaftParams

pytestmark = pytest.mark.gpu
PARAMS = RaftParams(est_cov=3, symmetric_mode=1)
ANCHOR = 300
# one record past a workgroup's 1024-record step and one past a lane's four: a larger stale staging behind a smaller live one
LARGE, MIDDLE, SMALL = 1025, 257, 5


def pass_columns():
    return overlaps_for([500, 77, 1200] * 5, 3)


def with_pass(engine):
    eng = engine.Engine(PARAMS, device=0)
    eng.run_host(*pass_columns())
    eng.finish()
    return eng


def test_host_forms_share_one_staging_set():
    from raft_amd import engine
    own_cols = [c[:SMALL] if k else c for k, c in enumerate(pass_columns())]        # five records over the pass's reads
    many = [rst_cases.case_reads()[1][rst_cases.R_130]] * 6 + [[]]                   # 780 runs: more than any call before it staged
    many_lens = rst_cases.i32(*[30000] * len(many))
    o_cols, o_rep = ovl_cases.stream(LARGE)
    f_cols, f_table, f_rep = frag_cases.stream(SMALL)
    r_cols, r_rep = rst_cases.stream(MIDDLE)
    r_cols = r_cols[:5] + [None, None]
    F_cols, F_table, F_rep = frag_cases.stream(LARGE)
    assert rst_cases.csr(many)[1].size > max(o_rep[1].size, f_rep[1].size, r_rep[1].size, f_table[1].size)
    eng = with_pass(engine)
    try:
        f = eng.fetch()
        own_rep = (f["rep_offset"], f["rep_s"], f["rep_e"])
        steps = [
            ("repeat_overlaps, 1025 records, given repeats", ovl_cases.same_classes,
             lambda e: e.repeat_overlaps(*o_cols, min_anchor=ANCHOR, repeats=o_rep), lambda: ovl_cases.want_classes(*o_cols, False, ANCHOR, *o_rep)),
            ("fragment_overlaps, 5 records, given table", frag_cases.same_fragments,
             lambda e: e.fragment_overlaps(*f_cols, fragments=f_table, repeats=f_rep), lambda: frag_cases.want_fragments(*f_cols, False, *f_table, *f_rep)),
            ("repeat_stats, 257 records, symmetric, no ts / te", rst_cases.same_stats,
             lambda e: e.repeat_stats(*r_cols, symmetric=True, repeats=r_rep, threshold=0), lambda: rst_cases.repeat_stats_model(*r_cols, True, *r_rep)),
            ("repeat_overlaps, 5 records, own pass", ovl_cases.same_classes,
             lambda e: e.repeat_overlaps(*own_cols, min_anchor=ANCHOR, symmetric=True), lambda: ovl_cases.want_classes(*own_cols, True, ANCHOR, *own_rep)),
            ("repeat_stats, no records, a larger table", rst_cases.same_stats,
             lambda e: e.repeat_stats(many_lens, repeats=rst_cases.csr(many), threshold=0),
             lambda: rst_cases.repeat_stats_model(many_lens, *[np.empty(0, np.int32)] * 6, False, *rst_cases.csr(many))),
            ("fragment_overlaps, 1025 records", frag_cases.same_fragments,
             lambda e: e.fragment_overlaps(*F_cols, fragments=F_table, repeats=F_rep), lambda: frag_cases.want_fragments(*F_cols, False, *F_table, *F_rep)),
        ]
        for what, same, call, model in steps:
            got = call(eng)
            same(got, model(), f"{what}: the model")
            fresh = with_pass(engine)
            try:
                same(got, call(fresh), f"{what}: a fresh context")
            finally:
                fresh.close()
        assert np.array_equal(eng.fetch()["cov"], f["cov"])                         # ... and the pass is as it was
    finally:
        eng.close()


# low_cov at which low_coverage reads int32 and not the pass's codes: any for int32 and four-bit steps, the code's limit or more for
# one and two bytes (300 keeps the deep windows of read 2 apart from the rest; above 65535 every window is low)
LOW_COV = {4: 3, 8: 3, 1: 300, 2: 70000}


@pytest.mark.parametrize("width", WIDTHS)
def test_queries_share_one_decoded_coverage(width):
    """low_coverage, repeat_stats, a smaller pass, low_coverage: nobody fetches, so a pass that wrote an encoding is decoded by each call
    into the pair the queries share."""
    from raft_amd import engine
    p = RaftParams(reso=RESO, est_cov=4, symmetric_mode=1)
    cols = window_set()
    small = overlaps_for([40, 7, 1, 0, 33], 6, reso=RESO)
    want, want_small = oracle_run(p, *cols), oracle_run(p, *small)
    assert want_small["cov"].size < want["cov"].size // 10
    rep = window_runs(cols[0], want["cov_offset"])
    low_cov = LOW_COV[width]
    eng = engine.Engine(p, device=0)
    try:
        eng.set_output_width(width)
        eng.run_host(*cols)
        eng.finish()
        same_low(eng.low_coverage(low_cov), want_low(want, cols[0], RESO, low_cov, 800), f"width {width}: low_coverage")
        cov = dict(threshold=5, cov_offset=want["cov_offset"], cov=want["cov"], reso=RESO)
        rst_cases.same_stats(eng.repeat_stats(*cols, symmetric=True, repeats=rep, threshold=5), rst_cases.repeat_stats_model(*cols, True, *rep, **cov),
                             f"width {width}: repeat_stats behind low_coverage")
        eng.run_host(*small)
        eng.finish()
        same_low(eng.low_coverage(low_cov), want_low(want_small, small[0], RESO, low_cov, 800), f"width {width}: low_coverage behind a smaller pass")
        got = eng.fetch()
        assert np.array_equal(got["cov"], want_small["cov"]) and np.array_equal(got["cov_offset"], want_small["cov_offset"])
    finally:
        eng.close()
