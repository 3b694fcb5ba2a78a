"""CPU: the tail sets of raft_testlib (the per-read tail of a pass, raft_amd/csrc/finalize.hpp, at its structural boundaries)
against the oracle -- and what keeps them honest.

For every set and parameter triple the oracle equals the closed form read by read: repeats as a set per read (the order under
ties is the oracle's, pinned to std::sort in test_oracle_golden.py), cut points, fragments and the three offset arrays exactly;
the closed form comes from tail_model, a plain restatement of chop.hpp:209-321.  A census made from the ORACLE's output and the
reads' places counts the reads of every class the sets aim at -- repeat counts on either side of 4 / 5, 16 / 17 and 24 / 25, tied
lanes per wave and waves per workgroup, kept markers on either side of div + 1, both remainders of (nF - 1) % div, flanked ends on
kL - 1, kL, kL + 1, the piece-edge classes, every N of tail_offsets -- and fails on an empty class.  The constants the sets are laid
on are read back from the sources.  Ten named wrong variants of tail_model, each one deliberate mistake, must each differ from the
oracle on a read of tail_markers, named by its coordinate.  tests/test_gpu_tail.py runs the same sets through the engine.
"""
import os
import re

import numpy as np
import pytest
import raft_testlib as T
from raft_testlib import (ROOT, RUN_Q, TAIL_COUNTS_FLANKS, TAIL_COUNTS_L, TAIL_DIVS, TAIL_FLANKS, TAIL_MARKERS_L, TAIL_NS, TAIL_PIECES_TRIPLES,
                          TAIL_VARIANTS, TILE_CAP, OracleError, TailFragmentError, assert_tail_result, oracle_run, tail_census,
                          tail_counts, tail_error_set, tail_first_difference, tail_markers, tail_model, tail_offsets, tail_overlaps, tail_pieces,
                          tail_shapes, tail_sort_hits_depth_limit)

CSRC = os.path.join(ROOT, "raft_amd", "csrc")


def check_closed_form(case, want):
    """The oracle against the construction, read by read; the totals the construction knows."""
    msg = tail_first_difference(case, case.expect, want, as_sets=True)
    assert msg is None, f"oracle against the closed form: {msg}"
    assert np.array_equal(case.expect["frag_read"], want["frag_read"]), case.name
    for k in ("total_repeat_length", "total_read_length"):
        assert case.expect[k] == want[k], (case.name, case.triple, k, case.expect[k], want[k])
    assert want["high_cov"] == 1 and case.expect["error_read"] == -1


def require(census, keys, what):
    missing = [k for k in keys if census.get(k, 0) < 1]
    assert not missing, f"{what}: no read in the classes {missing}"


def show(what, census):
    print(f"census {what}: " + ", ".join(f"{' '.join(str(x) for x in k)} = {v}" for k, v in census.items() if v))


MARKER_CLASSES = ([("nF - (div + 1)", d) for d in (-1, 0, 1)] + [("(nF - 1) % div", "zero"), ("len % L", "zero"), ("len % L", "non-zero"),
                                                                 ("len", "< L"), ("len", "== L"), ("len", "== 0")]
                  + [("s % L, e % L", a, b) for a in (TAIL_MARKERS_L - 1, 0, 1) for b in (TAIL_MARKERS_L - 1, 0, 1)]
                  + [("first marker inside a repeat",), ("last marker inside a repeat",), ("repeat", "covers no marker"),
                     ("repeat", "covers the last interior marker"), ("two repeats", "no marker between"), ("two repeats", "one marker apart")])


def test_the_constants_the_sets_are_built_on():
    fin, types, ctx, wl, eng, wave = (open(os.path.join(CSRC, f)).read() for f in
                                      ("finalize.hpp", "raft_types.hpp", "engine_ctx.hpp", "wave_launch.hpp", "engine.hip", "pileup_wave.hpp"))

    def one(pattern, text, count=1):
        m = re.findall(pattern, text)
        assert len(m) == count, (pattern, m)
        return m[0]
    assert int(one(r"\n    if \(n <= (\d+)\) \{ +// \(the reads without a repeat too", fin)) == T.TAIL_REG_N == 4          # RepReg / RepMem
    assert int(one(r"__ballot\(n > (\d+) && a\.raw_s\[base \+ 1\] == 0\)", fin)) == T.TAIL_TIE_N == 16                      # the tie order
    assert int(one(r"void sort_repeats\(int32_t \*k, int32_t \*s, int32_t \*e, int n\)\n\{\n    if \(n <= (\d+)\) \{", fin)) == T.TAIL_INSERTION_N == 24
    assert one(r"while \(last - first > (\d+)\)", fin) == "16" and one(r"if \(n > (\d+)\) \{\n        rep_insertion_sort\(v, 0, (\d+)\);", fin) == ("16", "16")
    for k in ("finalize_count_kernel", "finalize_cuts_kernel"):
        assert int(one(r"__global__ __launch_bounds__\((\d+)\) void " + k + r"\(FinalizeArgs a\)", fin)) == T.TAIL_WG == 256
    assert int(one(r"template <bool CUTS>\n__global__ __launch_bounds__\((\d+)\) void finalize_fill_kernel\(FinalizeArgs a\)", fin)) == T.TAIL_WG
    assert int(one(r"__global__ __launch_bounds__\((\d+)\) void tail_prefix_kernel\(", fin)) == T.TAIL_PREFIX_WG == 1024
    assert int(one(r"const int first = \(int\)blockIdx\.x \* (\d+), i = first", fin)) == T.TAIL_PREFIX_WG
    assert one(r"P\.tail_blocks = \(int\)std::max<long long>\(1, \(N \+ (\d+)\) / (\d+)\);", eng) == ("255", "256")
    assert one(r"hipLaunchKernelGGL\(tail_prefix_kernel, dim3\(\(unsigned\)\(\(P\.tail_blocks \+ (\d+)\) / (\d+)\)\), dim3\((\d+)\)", eng) == ("1023", "1024", "1024")
    assert T.TAIL_PREFIX_READS == 1024 * 256 == 262144 and T.TAIL_WAVE == 64
    assert int(one(r"constexpr int kRunQ = (\d+);", types)) == RUN_Q == 16
    one(r"if \(idx < kRunQ\) \{ sm\.runq\[idx \* 2\] = best; sm\.runq\[idx \* 2 \+ 1\] = t; \}\n +else emit_overflow\(best, t\);", wave)
    assert int(one(r"#define RAFT_WAVE_SLOTS (\d+)\b", wl)) - int(one(r"constexpr int kTileCap = kWaveSlots - (\d+);", ctx)) == TILE_CAP == 4092
    one(r"fa\.long_windows = kTileCap;", eng)
    one(r"const bool pieces = nb > a\.long_windows;", fin)


@pytest.mark.parametrize("div", TAIL_DIVS)
def test_markers(div, capsys):
    L = TAIL_MARKERS_L
    total = {}
    for flank in TAIL_FLANKS:
        for overlap in tail_overlaps(div, L):
            case = tail_markers(div, overlap, flank)
            want = case.oracle()
            check_closed_form(case, want)
            census = tail_census(case, want)
            keys = MARKER_CLASSES + ([("(nF - 1) % div", "non-zero")] if div > 1 else [])
            if flank:        # (runs are at least one low base apart: without a flank two repeats neither overlap nor share a marker)
                keys = keys + [("two repeats", "flanked intervals overlap"), ("two repeats", "share exactly one marker")]
            require(census, keys, f"tail_markers {case.triple}")
            for k, v in census.items():
                total[k] = total.get(k, 0) + v
            # every length 0 .. 3L + 1 and k*L + {-1, 0, 1} is there without a repeat
            bare = {int(case.cols[0][r]) for r in np.flatnonzero(np.diff(want["rep_offset"]) == 0)}
            assert bare >= set(range(0, 3 * L + 2)) | {k * L + d for k in (div, div + 1, div + 2, 2 * div, 2 * div + 1, 5 * div) for d in (-1, 0, 1)}
            assert 200 <= case.n_reads <= 1500
    with capsys.disabled():
        show(f"tail_markers div {div}, {len(TAIL_FLANKS) * 5} triples, {case.n_reads} reads each", total)


@pytest.mark.parametrize("flank", TAIL_COUNTS_FLANKS)
def test_counts(flank, capsys):
    for div in (1, 3):
        for overlap in (0, TAIL_COUNTS_L):
            case = tail_counts(div, overlap, flank)
            want = case.oracle()
            check_closed_form(case, want)
    census = tail_census(case, want)
    n = np.diff(want["rep_offset"])
    assert set(T.TAIL_COUNT_NS) <= set(n.tolist()) and 2 * 256 < case.n_reads <= 3 * 256
    keys = [("n", v) for v in (4, 5, 24, 25)] + [("n", 16, "tied"), ("n", 17, "tied"), ("last wave", "dead lanes behind a tied read"),
                                                  ("tied n > 24 next to tied n = 17", "same wave"), ("tied lanes in a wave", 64),
                                                  ("tied lanes in a wave", 2), ("waves of a workgroup with a tied lane", 4)]
    if flank == 8:           # the layout is made for this flank: a larger one ties every read of more than 16 repeats
        keys += [("n", 16, "untied"), ("n", 17, "untied"), ("tied lanes in a wave", 1), ("waves of a workgroup with a tied lane", 1),
                 ("ends not monotone",)]
        tied = (n > 16) & (want["rep_s"][np.minimum(want["rep_offset"][:-1] + 1, want["rep_s"].size - 1)] == 0) & (n >= 2)
        assert tied[:64].all() and np.flatnonzero(tied[64:128]).tolist() == [0, 63] and np.flatnonzero(tied[128:192]).tolist() == [17]
        assert n[128:192][np.arange(64) != 17].max() <= 4 and np.flatnonzero(tied[192:256]).tolist() == [5, 6] and n[197] > 24 and n[198] == 17
        # every repeat of a read has an end of its own: a wrong order among the tied entries shows
        for r in np.flatnonzero(tied):
            e = want["rep_e"][want["rep_offset"][r]:want["rep_offset"][r + 1]]
            assert np.unique(e).size == e.size, case.coordinate(r)
    if flank == 600:         # all of a read's repeats clamp to 0 with ends of their own: after the permutation one lies inside another
        keys += [("two repeats", "the second inside the first"), ("ends not monotone",)]
    require(census, keys, f"tail_counts flank {flank}")
    assert census[("run ends in 256 windows of a read", "max")] >= 2 * RUN_Q + 2      # whatever the half-rows' alignment, one closes more than kRunQ runs
    deep = sum(tail_sort_hits_depth_limit([s for s, _ in case.reps(r)]) for r in np.flatnonzero(n > 16))
    census[("introsort reached its depth limit", "reads")] = deep
    with capsys.disabled():
        show(f"tail_counts flank {flank}, {case.n_reads} reads", census)
        if not deep:
            print(f"census tail_counts flank {flank}: no read reaches the introsort depth limit (not required)")


def test_pieces(capsys):
    total = {}
    for triple in TAIL_PIECES_TRIPLES:
        case = tail_pieces(*triple)
        want = case.oracle()
        check_closed_form(case, want)
        for k, v in tail_census(case, want).items():
            total[k] = max(total.get(k, 0), v)
    require(total, [("piece", "a run crosses an edge"), ("piece", "one low window on an edge"), ("piece", "short parts join and reach repeat_length"),
                    ("piece", "short parts join one base short"), ("piece", "a run through a middle piece"), ("pieces", 2), ("pieces", 3), ("pieces", 4),
                    ("long read", "high windows, no repeat"), ("long read", "n == 4"), ("long read", "n == 5"), ("long read", "tied")], "tail_pieces")
    assert total[("long reads in one wave", "max")] >= 4
    W = np.diff(want["cov_offset"])
    long_ = np.flatnonzero(W > TILE_CAP)
    assert {int(r) // 256 for r in long_} == {0, 1} and np.sum(W <= 100) > 256      # long reads in both workgroups, among short ones
    # 4 joined from more raw records than 4, 5 joined: counted on the raw side as the parts of the runs between the piece edges
    for r in long_:
        if "joined from" in case.kind(r):
            joined, raw = (int(x) for x in re.match(r"(\d+) joined from (\d+) raw", case.kind(r)).groups())
            parts = sum(len(range(s // TILE_CAP, (e - 1) // TILE_CAP + 1)) for s, e in T._merge_runs(case.runs(r)))
            assert len(case.reps(r)) == joined == int(np.diff(want["rep_offset"])[r]) and parts == raw > joined
    with capsys.disabled():
        show(f"tail_pieces, {len(TAIL_PIECES_TRIPLES)} triples, {case.n_reads} reads", total)


@pytest.mark.parametrize("N", TAIL_NS)
def test_offsets(N, capsys):
    case = tail_offsets(N)
    want = case.oracle()
    check_closed_form(case, want)
    assert want["n_reads"] == N == case.n_reads and (N == 0 or case.cols[0].max() < 100)
    shape = tail_shapes(want)
    assert np.all(shape >= 0)
    if N >= 63:              # the first workgroup and the last two together hold all four shapes
        assert set(shape[:256].tolist()) == {0, 1, 2, 3} and set(shape[max((N - 1) // 256 - 1, 0) * 256:].tolist()) == {0, 1, 2, 3}
    if N >= 1024:            # the choice is not periodic in a wave or a workgroup
        assert not np.array_equal(shape[:64], shape[64:128]) and not np.array_equal(shape[:256], shape[256:512])
    with capsys.disabled():
        print(f"census tail_offsets N = {N}: reads per shape {np.bincount(shape, minlength=4).tolist()}, {int(want['cov_offset'][-1])} windows, "
              f"{want['rep_s'].size} repeats, {want['cuts'].size} cut points, {want['frag_read'].size} fragments")


def _model_result(case, variant):
    """What tail_model (or a wrong variant of it) gives for every read, in the oracle's layout; a read whose fragments are not
    defined gets none."""
    out = {"cut_offset": [0], "cuts": [], "frag_offset": [0], "frag_begin": [], "frag_end": []}
    for r in range(case.n_reads):
        reps = case.reps(r)
        runs = [(s, e) for (s, e) in T._merge_runs(case.runs(r)) if e - s >= case.p.repeat_length]
        try:
            F, frags = tail_model(case.length(r), reps, case.L, case.div, case.overlap, variant=variant, unflanked=runs)
        except (TailFragmentError, IndexError):
            F, frags = [], []
        out["cuts"] += F
        out["frag_begin"] += [b for b, _ in frags]
        out["frag_end"] += [e for _, e in frags]
        out["cut_offset"].append(len(out["cuts"]))
        out["frag_offset"].append(len(out["frag_begin"]))
    return {k: np.array(v, np.int64 if k.endswith("offset") else np.int32) for k, v in out.items()}


@pytest.mark.parametrize("variant", TAIL_VARIANTS)
def test_a_wrong_model_differs_on_a_named_read(variant, capsys):
    """The checks can fail: every variant -- one deliberate mistake each -- differs from the oracle on at least one read of
    tail_markers, and the message names that read by its coordinate.  (On the CPU only: no wrong kernel is built or run.)"""
    found = []
    for div in TAIL_DIVS:
        for flank in TAIL_FLANKS:
            for overlap in tail_overlaps(div, TAIL_MARKERS_L)[1:4:2] + (div * TAIL_MARKERS_L,):
                case = tail_markers(div, overlap, flank)
                want = case.oracle()
                assert tail_first_difference(case, _model_result(case, None), want) is None
                msg = tail_first_difference(case, _model_result(case, variant), want)
                if msg is not None:
                    m = re.search(r"\(div, overlap, flank\) = \((\d+), (\d+), (\d+)\), L = 10: read (\d+) \[([^\]]+)\] len (\d+), repeats (.*), lane (\d+), wave (\d+), workgroup (\d+)", msg)
                    assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == case.triple, msg
                    r = int(m.group(4))
                    assert case.kind(r) == m.group(5) and case.length(r) == int(m.group(6)) and (r % 64, r // 64, r // 256) == tuple(int(m.group(i)) for i in (8, 9, 10))
                    found.append(msg)
    assert found, f"variant '{variant}' agrees with the oracle on every read of tail_markers"
    with capsys.disabled():
        print(f"wrong model '{variant}': differs under {len(found)} of 24 triples; first: {found[0][:230]}")


@pytest.mark.parametrize("variant", T.TAIL_NO_MISTAKES)
def test_two_changes_that_are_no_mistakes(variant):
    """`nF <= div` as the whole-read test and `F[min(q + div, nF - 1)]` as the last fragment's end read like mistakes and change
    nothing (raft_testlib.TAIL_NO_MISTAKES says why): they agree with the oracle on every read.  Their wrong neighbours are among
    the variants above."""
    for div in TAIL_DIVS:
        case = tail_markers(div, 1, 2)
        assert tail_first_difference(case, _model_result(case, variant), case.oracle()) is None


def test_a_wrong_result_is_named_by_its_coordinate():
    case = tail_counts(3, 20, 8)
    want = case.oracle()
    n = np.diff(want["rep_offset"])
    r = 64 + 63                                               # wave 1, lane 63: 17 repeats, three of them clamped to 0
    assert n[r] == 17
    o = want["rep_offset"][r]
    bad = dict(want, rep_e=want["rep_e"].copy())
    bad["rep_e"][[o, o + 1]] = bad["rep_e"][[o + 1, o]]       # two tied entries the other way round
    with pytest.raises(AssertionError) as e:
        assert_tail_result(case, bad, want, "wave kernel, pass 1, cuts by the fill kernel")
    msg = str(e.value)
    assert msg.startswith("wave kernel, pass 1, cuts by the fill kernel: rep_e differs in 2 of") and \
        f"set tail_counts, (div, overlap, flank) = (3, 20, 8), L = 20: read {r} [n=17 k3] len {case.length(r)}, repeats 17:" in msg and \
        "lane 63, wave 1, workgroup 0" in msg
    bad = dict(want, frag_offset=want["frag_offset"].copy())
    bad["frag_offset"][300:] += 1                             # read 299 has one fragment more, every later offset moves
    with pytest.raises(AssertionError, match=r"number of fragments differs first in .*read 299 \[.*lane 43, wave 4, workgroup 1: got"):
        assert_tail_result(case, bad, want, "w")
    bad = dict(want, cuts=want["cuts"].copy())
    bad["cuts"][want["cut_offset"][5] + 1] += 1
    with pytest.raises(AssertionError, match=r"cuts differs in 1 of \d+ entries, first in .*read 5 \[.*at its entry 1"):
        assert_tail_result(case, bad, want, "w")
    # a result without cut points (a host pipeline's) is compared on what it holds
    part = {k: v for k, v in want.items() if k not in ("cuts", "cut_offset", "cov")}
    assert_tail_result(case, part, want, "w")
    # and the closed form is no echo of the oracle
    other = tail_counts(3, 0, 8)
    with pytest.raises(AssertionError, match="frag_begin differs"):
        check_closed_form(other, want)


def test_error_set():
    """Reads 3, 70, 300 and 700 alone would split: under overlap = div*L + 1 the oracle stops with FRAGMENT, the closed form names
    the first of them; with read 3 short, read 70; with all four short the set is defined."""
    for short, first in (((), 3), ((3,), 70), ((3, 70), 300), ((3, 70, 300), 700)):
        case = tail_error_set(short)
        assert case.expect["error_read"] == first and case.n_reads == 800
        with pytest.raises(OracleError) as e:
            case.oracle()
        assert e.value.code == 4
        legal = T.TailCase(case.name, T._tail_params(case.L, case.div, case.div * case.L, 0), case.templates, case.idx)
        want = legal.oracle()
        check_closed_form(legal, want)
        split = np.flatnonzero(np.diff(want["frag_offset"]) > 1).tolist()
        assert split == [r for r in T.TAIL_ERROR_READS if r not in short]
    case = tail_error_set(T.TAIL_ERROR_READS)
    check_closed_form(case, case.oracle())


def test_oracle_equals_the_reference_binary_on_the_tail_sets():
    """tests/golden/tail_ref.npz (make_tail_ref.py): tail_markers and a thinned tail_counts, regenerated with repeat_length = L as the
    command line ties them, through the unmodified reference binary."""
    n = T.tail_ref_count()
    assert n >= 40
    seen = set()
    for i in range(n):
        name, case, exp = T.tail_ref_case(i)
        cols = case.cols
        got = oracle_run(T.RaftParams(**dict(case.p.__dict__, symmetric_mode=-1)), *cols)
        T.assert_matches_ref_fuzz(got, exp, case.p, f"tail_ref case {i} ({name}, {case.triple})")
        msg = tail_first_difference(case, {k: v for k, v in got.items() if not k.startswith("cut")}, dict(exp, frag_offset=got["frag_offset"]))
        assert msg is None, msg
        seen.add((name, case.div))
    assert seen >= {("tail_markers", d) for d in TAIL_DIVS} | {("tail_counts", 1), ("tail_counts", 3)}
