"""CPU: the sets that tests/test_gpu_presplit_edges.py runs the pre-split job on (tests/presplit_cases.py) -- and what keeps them honest.

The two cut rules of raft_hip_run_presplit_local, the run limits, the rank limit and the grid cap of the mirror search are read back
from the sources, so that a changed rule fails here instead of moving an edge away from its case.  Every case's claims -- its classes,
the ranks without reads, the empty slices, the ranks that receive nothing, the runs that arrive -- are checked against the model; every
case is pinned to the oracle on the whole set; a census fails on an empty class."""
import os
import re

import numpy as np
import pytest
from presplit_cases import CASES, CLASSES, Model, case_id, holds, read_bounds, record_cut, sides_of
from raft_testlib import ROOT

CSRC = os.path.join(ROOT, "raft_amd", "csrc")


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def test_the_rules_the_cases_are_built_on():
    ex, ty = _src("engine_exchange.hip"), _src("raft_types.hpp")

    def count(pattern, text, n=1):
        m = re.findall(pattern, text)
        assert len(m) == n, (pattern, m)
        return m[0]
    # the record cut and the read bounds of the job (presplit_cases.record_cut / read_bounds restate them)
    count(r"const int64_t lo = n_rec \* r / world, hi = n_rec \* \(r \+ 1\) / world, n = hi - lo;", ex)
    count(r"win_off\[\(size_t\)i \+ 1\] = win_off\[\(size_t\)i\] \+ \(\(int64_t\)read_len\[i\] \+ reso - 1\) / reso;", ex)
    count(r"for \(int g = 1; g < world; \+\+g\)\n\s*bounds\[\(size_t\)g\] = std::lower_bound\(win_off\.begin\(\), win_off\.end\(\), \(int64_t\)\(\(__int128\)W \* g / world\)\) - win_off\.begin\(\);", ex)
    count(r"bounds\[\(size_t\)world\] = n_reads;\n\s*for \(int g = 1; g <= world; \+\+g\) bounds\[\(size_t\)g\] = "
          r"std::min<int64_t>\(std::max\(bounds\[\(size_t\)g\], bounds\[\(size_t\)g - 1\]\), n_reads\);", ex)
    # the error index of the job is the same cut plus the slice's own index
    count(r"summary->error_index = n_rec \* r / world \+ ctxs\[r\]->gs_err_index;", ex)
    # runs: a slice has at most kMaxSeg, a rank receives at most kMaxRuns
    assert count(r"constexpr int kMaxSeg = (\d+);", ty) == "4" and count(r"constexpr int kMaxRuns = (\d+);", ty) == "16"
    count(r"sl\.n_runs >= 1 && sl\.n_runs <= kMaxSeg", ex)
    count(r"if \(\(int\)runs\.size\(\) > kMaxRuns\) \{ c->last_error = \"raft_hip_exchange: more than 16 runs arrive at one rank\"; return RAFT_HIP_ERR_TOO_LARGE; \}", ex)
    count(r"if \(arriving > kMaxRuns\) \{", ex)
    # ranks of one process; the mirror search's grid (256 threads, at most 256 * 16 blocks: beyond 256 * 256 * 16 records a thread strides)
    count(r"if \(!ctxs \|\| world < 1 \|\| world > (64) \|\| n_reads < 0 \|\| n_rec < 0 \|\| !out\) return RAFT_HIP_ERR_PARAM;", ex)
    count(r"mirror_search_kernel, dim3\(\(unsigned\)std::min<long long>\(\(r\.n_rec \+ 255\) / 256, 256 \* 16\)\), dim3\(256\)", ex)
    count(r"for \(long long i = \(long long\)blockIdx\.x \* blockDim\.x \+ threadIdx\.x; i < n_rec; i \+= \(long long\)gridDim\.x \* blockDim\.x\)\n\s*hit \|= i != first_index", ex)
    # record 0 and the column form are the first non-empty slice's, not rank 0's
    count(r"for \(int p = 0; p < world && first < 0; \+\+p\) if \(slices\[p\]\.n_rec > 0\) first = p;", ex)
    count(r"for \(int p = 0; p < world && first < 0; \+\+p\) if \(rows\[kRow \* \(size_t\)p \+ 6\] == 1\) first = p;", ex)
    count(r"for \(int p = 0; p < world && form_of < 0; \+\+p\) if \(slices\[p\]\.n_rec > 0\) form_of = p;", ex)
    # the model itself, on the examples the rules were described with
    assert read_bounds([100, 100], 50, 3) == [0, 1, 1, 2] and read_bounds([50, 100000, 50], 50, 4) == [0, 2, 2, 2, 3]
    assert read_bounds([0, 0, 0, 0], 50, 3) == [0, 0, 0, 4] and read_bounds([], 50, 3) == [0, 0, 0, 0]
    assert record_cut(2, 3) == [0, 0, 1, 2] and record_cut(0, 2) == [0, 0, 0] and record_cut(4, 3) == [0, 1, 2, 4]


def test_census_every_class_is_filled():
    filled = {}
    for case in CASES:
        for c in case.classes:
            filled.setdefault(c, []).append(case.name)
    missing = [c for c in CLASSES if not filled.get(c)]
    assert not missing, f"no case in the classes {missing}"
    assert set(filled) - {f"world={w}" for w in range(65)} <= set(CLASSES), set(filled) - set(CLASSES)
    assert len({c.name for c in CASES}) == len(CASES)
    # tiny: at most 64 reads and a few hundred records (the two sets with 255 intervals on a window need theirs)
    for case in CASES:
        assert case.read_len.size <= 64 and case.n_rec <= (600 if case.widths != (1,) else 300) and 1 <= case.world <= 64, case.name


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_claims_hold_in_the_model_and_the_oracle_runs(case):
    m = Model(case)
    for c in case.classes:
        assert holds(c, case, m), (case.name, c)
    assert m.no_reads == case.no_reads, ("ranks without reads", m.bounds)
    assert m.empty_slices == case.empty_slices, ("empty slices", m.cut)
    assert m.receives_nothing == case.receives_nothing and m.runs == case.runs, ("runs arriving", m.runs)
    assert max(m.runs, default=0) <= 16 and int(m.symmetric) == case.symmetric
    cols = case.cols
    assert all(a.dtype == np.int32 and a.shape == (case.n_rec,) for a in cols) and case.read_len.dtype == np.int32
    want = case.oracle()
    assert want["symmetric"] == case.symmetric and want["n_reads"] == case.read_len.size
    assert want["n_intervals"] == len(sides_of(case.recs, m.symmetric)) == sum(m.n_intervals)
    assert np.array_equal(want["cov_offset"], np.asarray(m.prefix, np.int64))
    # the ranks' shares add up to the whole: every interval lies on a read of the rank that the model routes it to
    for g in range(case.world):
        lo, hi = m.prefix[m.bounds[g]], m.prefix[m.bounds[g + 1]]
        assert (int(want["cov"][lo:hi].sum()) > 0) == (m.n_intervals[g] > 0), (case.name, g)
