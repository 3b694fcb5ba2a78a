"""CPU: the sets that tests/test_gpu_exc_capacity.py puts on either side of every exception list's first size (raft_testlib
exc_capacity_cases) -- and what keeps them honest.

The first sizes and the six comparisons between a count and a capacity are read back from the sources, so that a changed size or a
rewritten comparison fails here instead of moving the boundary away from the cases.  Every set's closed forms -- the coverage, and
the list an encoding must hold -- are pinned to the oracle; a census over (width, route, arm of the first size, K - cap0) fails on an
empty class; the host's encoders and decoders round-trip every set."""
import os
import re

import numpy as np
import pytest
from raft_testlib import (EXC_B_ARM, EXC_CAP_FLOOR, EXC_LIMIT, ROOT, delta4_reference, exc_cap0, exc_capacity_case, exc_capacity_list, exc_case_id,
                          exc_classes, exc_closed_list)

CSRC = os.path.join(ROOT, "raft_amd", "csrc")
HOST = os.path.join(ROOT, "raft_amd", "host")


def _src(d, name):
    return open(os.path.join(d, name)).read()


def test_the_sizes_and_comparisons_the_cases_are_built_on():
    en, pk, pl, cp = _src(CSRC, "engine.hip"), _src(CSRC, "pack.hpp"), _src(CSRC, "engine_pipeline.hip"), _src(HOST, "cli_plan.hpp")

    def count(pattern, text, n=1):
        m = re.findall(pattern, text)
        assert len(m) == n, (pattern, m)
        return m[0]
    # the first sizes
    assert count(r"const long long cap = std::max<long long>\(c->exc_cap, std::max<long long>\((\d+), B / (\d+)\)\);", en) == ("4096", "64")
    assert count(r"long long cap = std::max<long long>\(c->exc_cap, std::max<long long>\((\d+), d4 \? B / (\d+) : B / (\d+)\)\);", en) == ("4096", "64", "512")
    assert count(r"c\.exc_cap0 = std::max<int64_t>\(1 << (\d+), c\.n_win / (\d+)\);", cp) == ("16", "64")
    assert (exc_cap0("pass", 1, 64 * 4096 - 1), exc_cap0("pass", 2, 64 * 4097), exc_cap0("reencode", 8, 64 * 4097)) == (4096, 4097, 4097)
    assert (exc_cap0("reencode", 1, 64 * 4097), exc_cap0("reencode", 2, 512 * 4097), EXC_CAP_FLOOR, EXC_B_ARM) == (4096, 4097, 4096, 4100)
    # the limits
    assert count(r"struct PackLimit<uint8_t> \{ static constexpr unsigned value = (\d+)u; \}", pk) == "255" and EXC_LIMIT[1] == 255
    assert count(r"struct PackLimit<uint16_t> \{ static constexpr unsigned value = (\d+)u; \}", pk) == "65535" and EXC_LIMIT[2] == 65535
    count(r"if \(!force && \(unsigned\)\(step \+ 7\) <= 14u\) return", pk)
    # the six comparisons (DESIGN.md names the test that holds each)
    count(r"if \(\(long long\)slot < o\.exc_cap\) \{ o\.exc_idx\[slot\] = ", pk, 2)
    count(r"if \(at < exc_cap\) \{ exc_idx\[at\] = ", pk)
    count(r"c->pass_width != 4 && \(long long\)hc\.n_exc > c->exc_cap && ", en)
    count(r"if \(c->n_exc <= cap\) break;", en)
    count(r"if \(c->n_exc > exc_cap && \(cov_packed \|\| exc_index \|\| exc_value\)\) return RAFT_HIP_ERR_TOO_LARGE;", en)
    count(r"exc_fits = b_exc \+ (?:cr->)?n_exc <= o->exc_cap;", pl, 2)
    count(r"if \(o->n_exc > o->exc_cap\) \{", pl)
    count(r"return rc != RAFT_HIP_ERR_TOO_LARGE \|\| attempt == 2 \|\| n_exc <= exc_cap;", cp)
    # a context's capacity only grows, and is kept across passes
    count(r"c->exc_cap = cap;", en, 2)
    count(r"c->exc_cap = \(long long\)hc\.n_exc;", en)
    # the deep kernel's tile list: 1024 tiles before a pass is run again for ITS sake (the sets stay below)
    assert count(r"long long deep_cap = (\d+);", _src(CSRC, "engine_ctx.hpp")) == "1024"


BOUNDARY, SMALL = exc_capacity_list(), exc_capacity_list("small")


def test_census_every_class_is_filled():
    classes = {}
    for spec in BOUNDARY:
        width, geometry, K, B = spec
        for c in exc_classes(width, K, B):
            classes.setdefault(c, []).append(exc_case_id(spec))
    want = [(w, r, arm, d) for w, r, arms in ((1, "pass", ("4096", "B/64")), (2, "pass", ("4096", "B/64")), (1, "reencode", ("4096", "B/512")),
                                              (2, "reencode", ("4096", "B/512")), (8, "reencode", ("4096", "B/64")))
            for arm in arms for d in (-1, 0, 1)]
    missing = [c for c in want if not classes.get(c)]
    assert not missing, f"no case in the classes {missing}"
    assert set(classes) == set(want)
    # both geometries of the byte lists in every byte class; short reads under the two-byte limit at least once
    for c, ids in classes.items():
        if c[0] == 1:
            assert {i.split("-")[1] for i in ids} == {"short", "long"}, (c, ids)
    assert any(s[0] == 2 and s[1] == "short" for s in BOUNDARY)
    assert {(s[0], s[2]) for s in SMALL} == {(w, K) for w in (1, 2, 8) for K in (0, 1, 2)}
    # every B sits clearly on its arm: never where both arms give the same size
    for width, geometry, K, B in BOUNDARY:
        assert B // 64 != EXC_CAP_FLOOR and B // 512 != EXC_CAP_FLOOR and B >= K, (width, geometry, K, B)


@pytest.mark.parametrize("spec", BOUNDARY + SMALL, ids=exc_case_id)
def test_closed_forms_equal_the_oracle_and_round_trip(spec):
    from raft_amd import hostio
    width, geometry, K, B = spec
    case = exc_capacity_case(*spec)
    assert (case.width, case.K, case.B) == (width, K, B) and case.expect.size == K and case.classes() == exc_classes(width, K, B)
    assert all(a.dtype == np.int32 for a in case.cols) and np.all(np.diff(case.cols[1]) >= 0)
    want = case.oracle()
    assert np.array_equal(want["cov_offset"], case.cov_offset) and np.array_equal(want["cov"], case.cov)
    assert np.array_equal(exc_closed_list(want["cov"], width), case.expect) and np.all(np.diff(case.expect) > 0)
    cov = want["cov"]
    if width == 8:
        nib, anchor, xi, xv = delta4_reference(cov)
        assert np.array_equal(xi, case.expect) and np.array_equal(xv, cov[case.expect])
        assert np.array_equal(hostio.unpack_coverage_d4(B, nib, anchor, xi, xv), cov)
        if K:                                            # (one entry short: the decoder refuses, or cannot restore the array -- the list is needed in full)
            try:
                short = hostio.unpack_coverage_d4(B, nib, anchor, xi[:-1], xv[:-1])
            except hostio.HostError:
                short = None
            assert short is None or not np.array_equal(short, cov)
    else:
        code, xi, xv = hostio.pack_coverage(cov, width)
        assert code.dtype == (np.uint8 if width == 1 else np.uint16)
        assert np.array_equal(xi, case.expect) and np.array_equal(xv, cov[case.expect]) and int(xv.min(initial=1 << 30)) >= EXC_LIMIT[width]
        assert int(xv.max(initial=0)) > EXC_LIMIT[width] or K < 3                # (values beyond the limit itself, not only at it)
        assert np.array_equal(hostio.unpack_coverage(code, xi, xv), cov)
        if K:
            assert not np.array_equal(hostio.unpack_coverage(code, xi[:-1], xv[:-1]), cov) or int(xv[-1]) == EXC_LIMIT[width]
    if width == 2:                   # (nothing between the two limits: the byte list of a two-byte set holds the same K windows)
        assert int((cov >= 255).sum()) == K
