"""CPU: the case list of tests/test_gpu_read_stats.py, built from the structural constants of raft_amd/csrc/read_stats.hpp (read back
from the header), with a census taken from the cases alone -- every class of segment shape the kernel treats differently must be
present, for both span sizes (2048 windows of int32 / uint16 codes, 4096 of byte codes) -- and raft_host_write_read_stats against a
restatement of its line format."""
import ctypes as C
import os
import re

import numpy as np
from raft_testlib import ROOT

RESO = 50


def constants():
    """kReadStats* of read_stats.hpp and, per output width (4: int32, also what delta4 is decoded into; 2; 1), the windows of one lane
    group and of one span."""
    text = open(os.path.join(ROOT, "raft_amd", "csrc", "read_stats.hpp")).read()
    k = {name: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
         for name in ("kReadStatsThreads", "kReadStatsInFlight", "kReadStatsSpanGroups", "kReadStatsSlots", "kReadStatsMaxBlocks")}
    vecs = {t: int(v) for t, v in re.findall(r"struct ReadStatsIn<(\w+)> \{ static constexpr int vecs = (\d+);", text)}
    lane_windows = {4: vecs["int32_t"] * 16 // 4, 2: vecs["uint16_t"] * 16 // 2, 1: vecs["uint8_t"] * 16}
    k["lane_windows"] = lane_windows
    k["span"] = {w: k["kReadStatsSpanGroups"] * lw for w, lw in lane_windows.items()}
    return k


def segment_cases():
    """name -> windows of every read, in order."""
    k = constants()
    T, cap = k["kReadStatsSlots"], k["kReadStatsMaxBlocks"]
    spans = sorted(set(k["span"].values()))
    cases = {f"one_read_of_{n}": [n] for n in (1, 5, 7, 9, 17, 35)}
    for r in range(16):                                   # n_bins = 32 + r: every residue modulo 16, tails shorter than a lane group
        cases[f"residue_{r}"] = [20, 12 + r]
    cases["empty_read_between"] = [5, 0, 7]
    cases["empty_reads_at_both_ends"] = [0, 0, 9, 0]
    for n in (T - 1, T, T + 1, 3 * T):                    # more reads in a span than the table has slots: the table loop iterates
        cases[f"one_window_run_{n}"] = [100] + [1] * n + [100]
    cases["empty_run_longer_than_the_table"] = [3] + [0] * (T + 5) + [4]
    for S in spans:
        cases[f"read_of_one_span_{S}"] = [S, 5]
        cases[f"begins_one_before_the_boundary_{S}"] = [S - 1, 10]
        cases[f"ends_one_after_the_boundary_{S}"] = [S + 1, 10]
        cases[f"more_than_three_spans_{S}"] = [2, 3 * S + 50, 2]
    big = max(spans)
    cases["grid_stride"] = [40000] * ((cap * big) // 40000 + 2)      # more spans than the capped grid takes in one step, in every width
    return cases


def overlaps_for(windows, seed, per_read=3, reso=RESO):
    """Reads of the given window counts (0: a read of length 0) with a few random self overlaps each."""
    rng = np.random.default_rng(seed)
    W = np.asarray(windows, np.int64)
    rl = np.where(W > 0, W * reso - rng.integers(0, reso, W.size), 0).astype(np.int32)
    per = per_read if W.size < 1000 else 1
    qid = np.repeat(np.flatnonzero(W > 0), per).astype(np.int32)
    a = (rng.random(qid.size) * rl[qid]).astype(np.int32)
    b = np.minimum(rl[qid], a + 1 + (rng.random(qid.size) * rl[qid]).astype(np.int32)).astype(np.int32)
    return [rl, qid, a, b, qid.copy(), a.copy(), b.copy()]


def census(windows, S, k):
    """The classes of one case under span S, from the window counts alone."""
    T, cap = k["kReadStatsSlots"], k["kReadStatsMaxBlocks"]
    W = np.asarray(windows, np.int64)
    off = np.concatenate([[0], np.cumsum(W)])
    n_bins = int(off[-1])
    begin, end = off[:-1], off[1:]
    out = set()
    if n_bins == 0:
        return {"no_windows"}
    out.add(f"residue_{n_bins % 16}")
    if 0 < n_bins % 16 < 8:
        out.add("tail_shorter_than_a_lane_group")
    if (W == 0).any():
        out.add("empty_read")
    if (W == 1).any():
        out.add("one_window_read")
    n_spans = -(-n_bins // S)
    if n_spans > cap:
        out.add("grid_stride_iterates")
    first_span, last_span = begin // S, (end - 1) // S
    reads_in_span = np.bincount(np.concatenate([first_span[W > 0], last_span[W > 0]]))  # (a lower bound: enough for the runs below)
    for n in (T - 1, T, T + 1, 3 * T):
        # a span that holds exactly n one-window reads in a row (plus the reads around them)
        ones = (W == 1)
        runs = np.diff(np.flatnonzero(np.diff(np.concatenate([[0], ones.astype(np.int8), [0]])) != 0))[::2] if ones.any() else []
        if any(int(r) == n for r in runs) and n_spans == 1:
            out.add(f"one_window_run_{n}")
    if reads_in_span.size and (np.bincount(first_span[W > 0]).max() > T):
        out.add("more_reads_than_slots")
    if ((W == 0).astype(np.int64).sum() > T):
        out.add("more_empty_reads_than_slots")
    nz = W > 0
    if ((begin[nz] % S == 0) & (W[nz] == S)).any():
        out.add("read_of_one_span")
    if (begin[nz] % S == S - 1).any():
        out.add("begins_one_before_a_boundary")
    if (end[nz] % S == 1).any() and (W[nz][end[nz] % S == 1] > 1).any():
        out.add("ends_one_after_a_boundary")
    if ((last_span - first_span)[nz] >= 3).any():
        i = int(np.flatnonzero(nz & (last_span - first_span >= 3))[0])
        if 0 < i < W.size - 1 and W[i - 1] == 2 and W[i + 1] == 2:
            out.add("more_than_three_spans_between_two_small_reads")
    if ((first_span == last_span) & nz & (begin > 0) & (end < n_bins)).any():
        out.add("read_wholly_inside_a_span")
    if ((first_span != last_span) & nz).any():
        out.add("read_across_spans")
    return out


REQUIRED = ({f"residue_{r}" for r in range(16)} |
            {"tail_shorter_than_a_lane_group", "empty_read", "one_window_read", "grid_stride_iterates", "more_reads_than_slots",
             "more_empty_reads_than_slots", "read_of_one_span", "begins_one_before_a_boundary", "ends_one_after_a_boundary",
             "more_than_three_spans_between_two_small_reads", "read_wholly_inside_a_span", "read_across_spans"})


def test_constants_are_what_the_cases_assume():
    k = constants()
    assert k["kReadStatsSpanGroups"] == k["kReadStatsThreads"] * k["kReadStatsInFlight"]
    assert k["lane_windows"] == {4: 8, 2: 8, 1: 16} and k["kReadStatsSlots"] >= 2
    for S in k["span"].values():
        assert 3 * k["kReadStatsSlots"] + 200 < S          # the runs of one-window reads lie inside one span


def test_every_class_is_present_for_every_span():
    k = constants()
    cases = segment_cases()
    for S in sorted(set(k["span"].values())):
        seen = set()
        for name, windows in cases.items():
            seen |= census(windows, S, k)
        need = REQUIRED | {f"one_window_run_{n}" for n in (k["kReadStatsSlots"] - 1, k["kReadStatsSlots"], k["kReadStatsSlots"] + 1, 3 * k["kReadStatsSlots"])}
        assert not (need - seen), (S, sorted(need - seen))


def test_overlaps_for_gives_the_window_counts():
    for name, windows in segment_cases().items():
        if name == "grid_stride":
            continue
        rl = overlaps_for(windows, 1)[0]
        assert np.array_equal((rl.astype(np.int64) + RESO - 1) // RESO, np.asarray(windows)), name


# ---- raft_host_write_read_stats ---------------------------------------------------------------------------------------------------------

def restate_tsv(names, length, reso, intervals, contained, cov_sum, cov_max, high_windows, rep_offset, frag_offset):
    lines = ["read\tname\tlength\twindows\tintervals\tcontained\tcov_sum\tcov_max\thigh_windows\trepeats\tfragments"]
    for i, nm in enumerate(names):
        lines.append("\t".join(str(x) for x in (i, nm, int(length[i]), (int(length[i]) + reso - 1) // reso, int(intervals[i]), int(contained[i]),
                                                 int(cov_sum[i]), int(cov_max[i]), int(high_windows[i]), int(rep_offset[i + 1] - rep_offset[i]),
                                                 int(frag_offset[i + 1] - frag_offset[i]))))
    return "\n".join(lines) + "\n"


def test_host_writer_against_the_line_format(tmp_path):
    from raft_amd import hostio
    lib = hostio.load_library()
    names = ["r0", "read/1 with_odd-chars", "x", "empty"]
    length = np.array([1234, 50, 99999, 0], np.int32)
    intervals = np.array([3, 0, 2147483647, 0], np.int32)
    contained = np.array([0, 1, 3, 2], np.uint8)
    cov_sum = np.array([17, 0, 2 ** 40 + 5, 0], np.int64)
    cov_max = np.array([9, 0, 2 ** 31 - 1, 0], np.int32)
    high = np.array([1, 0, 2000, 0], np.int32)
    rep_off = np.array([0, 2, 2, 7, 7], np.int64)
    frag_off = np.array([0, 1, 2, 9, 9], np.int64)
    for reso in (50, 1, 1000):
        path = str(tmp_path / f"t{reso}.tsv")
        arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
        P = lambda a: C.c_void_p(a.ctypes.data)
        rc = lib.raft_host_write_read_stats(path.encode(), len(names), arr, P(length), reso, P(intervals), P(contained), P(cov_sum), P(cov_max),
                                            P(high), P(rep_off), P(frag_off))
        assert rc == 0
        assert open(path).read() == restate_tsv(names, length, reso, intervals, contained, cov_sum, cov_max, high, rep_off, frag_off)
    rc = lib.raft_host_write_read_stats(str(tmp_path / "no_such_dir" / "x.tsv").encode(), len(names), arr, P(length), 50, P(intervals), P(contained),
                                        P(cov_sum), P(cov_max), P(high), P(rep_off), P(frag_off))
    assert rc != 0
