"""GPU: every rung of the `raft` command line's ladder behind an overflowing exception list (raft_main.cpp run_engine, cli_plan.hpp
next_attempt / ladder_stops / cov_bytes_needed), end to end.

    one byte -> two bytes          more than one window in 16 at or above 255
    four-bit steps -> two bytes    more than one window in 8 whose step leaves +-7
    four-bit steps -> longer list  more than the first size, fewer than one window in 8
    exactly at the first size      65,535 and 65,536 windows at or above 255 are held by the first attempt; 65,537 are not
(one byte -> longer list: tests/test_gpu_cli.py test_cli_encoding_ladder.)  A rung to two bytes per window needs twice the bytes of
the coverage array that were page-locked beside the tokenising: every run is made as it is and with RAFT_NO_PIN=1, and both must
agree.  Every case first shows, from the oracle's coverage, that the set takes the rung it claims; then the stage clock's
`coverage_encoding` and `attempts`, exit status 0, and the four files against the oracle's arrays and, where it is built, the
reference binary's files.

Left out: two bytes -> longer list, and a third attempt (one byte -> two bytes -> longer list).  Both need more than 65,536 windows
65,535 deep -- some 4e9 increments of the oracle's pileup, too slow for a test; the decisions stay with tests/cli_plan_check.cpp."""
import os
import subprocess

import numpy as np
import pytest
from raft_testlib import (RaftParams, assert_same_result, have_ref_bin, md5, oracle_run, result_from_ref_files, run_ref_binary, write_fasta,
                          write_paf)
from test_gpu_cli import RAFT, strip_timing

pytestmark = pytest.mark.gpu

FILES = ("reads.fasta", "coverage.txt", "long_repeats.txt", "long_repeats.bed")
FIRST_SIZE = 65536                 # cli_plan.hpp output_capacities: exc_cap0 = max(1 << 16, n_win / 64)


def raft_twice(tmp_path, args, env):
    """The run as it is and with the host arrays left pageable: -> (stdout, stderr) of the first, after showing that both agree."""
    runs = []
    for prefix, extra in (("out", {}), ("nopin", {"RAFT_NO_PIN": "1"})):
        r = subprocess.run([RAFT] + args + ["-o", prefix, "reads.fa", "overlaps.paf"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300,
                           env=dict(os.environ, RAFT_TIMING="1", **env, **extra))
        out, err = r.stdout.decode(), r.stderr.decode()
        assert r.returncode == 0, (prefix, out[-2000:] + err[-2000:])
        runs.append((out, err))
    labels = [[l for l in err.splitlines() if l.startswith(("TIMING devices_used", "TIMING coverage_encoding"))] for _, err in runs]
    assert labels[0] == labels[1] and len(labels[0]) == 2, labels
    assert strip_timing(runs[0][0]) == strip_timing(runs[1][0])
    for f in FILES:
        assert md5(open(tmp_path / ("out." + f), "rb").read()) == md5(open(tmp_path / ("nopin." + f), "rb").read()), f
    return runs[0]


def attempts_of(err):
    line = [l for l in err.splitlines() if l.startswith("TIMING devices_used")]
    assert len(line) == 1 and line[0].split()[-2] == "attempts", err
    return int(line[0].split()[-1])


def check_against_oracle(tmp_path, name, p, cols, names, out, want, ref_args):
    """The four files as CSR arrays, and what stdout says, against the oracle (as test_cli_encoding_ladder does); the reference
    binary's files where it is built."""
    rl = cols[0]
    got = result_from_ref_files(str(tmp_path / "out"), names)
    lines = out.split("\n")
    got.update(symmetric=int("INFO, Symmetric overlaps 1 " in lines), high_cov=int([l for l in lines if l.startswith("high_cov ")][0].split()[1]),
               total_windows=got["cov"].size, total_coverage=int(got["cov"].sum(dtype=np.int64)), total_read_length=int(rl.sum(dtype=np.int64)))
    got.update(cut_offset=want["cut_offset"], cuts=want["cuts"], total_repeat_length=want["total_repeat_length"])   # (in no file as integers)
    assert "fraction_of_repeat_length %f \n" % (want["total_repeat_length"] / want["total_read_length"]) in out
    assert "coverage per window is %f \n" % (want["total_coverage"] / want["total_windows"]) in out
    assert_same_result(got, want, name)
    if have_ref_bin():
        rc, ref_out = run_ref_binary(str(tmp_path), ref_args + ["-o", "ref"], "reads.fa", "overlaps.paf")
        assert rc == 0, ref_out[-400:]
        for f in FILES:
            assert md5(open(tmp_path / ("out." + f), "rb").read()) == md5(open(tmp_path / ("ref." + f), "rb").read()), (name, f)
        assert strip_timing(out) == strip_timing(ref_out.decode())


def write_inputs(tmp_path, cols):
    names = [f"r{i}" for i in range(cols[0].size)]
    write_fasta(tmp_path / "reads.fa", names, cols[0])
    write_paf(tmp_path / "overlaps.paf", names, *cols)
    return names


def byte_set(lens):
    """256 records 0 -> 1 over the whole of both reads and their 256 mirrors: every window of reads 0 and 1 sits at 256."""
    rl = np.array(lens, np.int32)
    qid = np.repeat(np.array([0, 1], np.int32), 256)
    tid = 1 - qid
    zero = np.zeros(qid.size, np.int32)
    return [rl, qid, zero, rl[qid], tid, zero, rl[tid]]


def test_one_byte_to_two_bytes(tmp_path):
    """-r 1 -e 30, RAFT_NO_DELTA4=1: 132,000 of 132,300 windows at 256 -- more than the first size and more than one in 16.  The
    second attempt's two bytes per window do not fit the range that was page-locked for one: the array is registered anew."""
    cols = byte_set([66000, 66000, 100, 100, 100])
    p = RaftParams(reso=1, est_cov=30)
    want = oracle_run(p, *cols)
    n_win, n_exc = int(want["cov"].size), int((want["cov"] >= 255).sum())
    assert (n_win, n_exc) == (132300, 132000) and max(FIRST_SIZE, n_win // 64) == FIRST_SIZE < n_exc and n_exc > n_win // 16
    assert int((want["cov"] >= 65535).sum()) == 0
    names = write_inputs(tmp_path, cols)
    out, err = raft_twice(tmp_path, ["-r", "1", "-e", "30"], {"RAFT_NO_DELTA4": "1"})
    assert "TIMING coverage_encoding uint16\n" in err and attempts_of(err) == 2, err
    check_against_oracle(tmp_path, "one byte -> two bytes", p, cols, names, out, want, ["-r", "1", "-e", "30"])


def step_set(n_groups, cold_windows, reso=50):
    """One-window reads 8 deep -- mirrored pairs (a, b): eight records a -> b and eight b -> a, no self overlaps --, each followed
    by an uncovered read of `cold_windows` windows.  Sorted by query: the shape of a hifiasm PAF, which the CLI answers in four-bit
    steps.  Every hot window is a step of +8 and the window behind it one of -8."""
    assert n_groups % 2 == 0
    rl = np.tile(np.array([reso, cold_windows * reso], np.int32), n_groups)
    rl = np.concatenate([np.array([cold_windows * reso], np.int32), rl])           # (an uncovered read first: the first window is no step)
    hot = 1 + 2 * np.arange(n_groups, dtype=np.int32)
    mate = hot.reshape(-1, 2)[:, ::-1].reshape(-1)
    qid, tid = np.repeat(hot, 8), np.repeat(mate, 8)
    zero = np.zeros(qid.size, np.int32)
    return [rl, qid, zero, rl[qid], tid, zero, rl[tid]]


def test_four_bit_steps_to_two_bytes(tmp_path):
    """-e 30: 66,004 windows alternately 8 deep and uncovered -- every step is +-8: more than the first size and more than one window
    in 8.  Four-bit steps that mostly do not fit are given up for two bytes per window, which -e below 40 did not page-lock."""
    cols = step_set(33002, 1)
    p = RaftParams(est_cov=30)
    want = oracle_run(p, *cols)
    cov = want["cov"].astype(np.int64)
    n_win, n_steps = int(cov.size), int((np.abs(np.diff(np.concatenate([[0], cov]))) > 7).sum())
    assert want["symmetric"] == 1 and n_win == 66005 and n_steps == 66004 > max(FIRST_SIZE, n_win // 64) == FIRST_SIZE and n_steps > n_win // 8
    names = write_inputs(tmp_path, cols)
    out, err = raft_twice(tmp_path, p.cli_args(), {})
    assert "derived by the engine" in err and "TIMING coverage_encoding uint16\n" in err and attempts_of(err) == 2, err
    check_against_oracle(tmp_path, "four-bit steps -> two bytes", p, cols, names, out, want, p.cli_args())


def test_four_bit_steps_to_a_longer_list(tmp_path):
    """-e 30: 33,100 one-window reads 8 deep, each between uncovered reads of 16 windows: 66,200 large steps (and a first window per
    tile) among 562,716 windows -- more than the first size, fewer than one window in 8: the second attempt keeps the four-bit steps
    and brings a list of exactly the length the first reported."""
    cols = step_set(33100, 16)
    p = RaftParams(est_cov=30)
    want = oracle_run(p, *cols)
    cov = want["cov"].astype(np.int64)
    n_win, n_steps = int(cov.size), int((np.abs(np.diff(np.concatenate([[0], cov]))) > 7).sum())
    # (the engine lists a first window per tile too: a tile holds up to 63 reads and 4092 windows -- with twice as many tiles as
    # that takes, the list still stays below one window in 8)
    n_tiles = cols[0].size // 63 + n_win // 4092
    assert want["symmetric"] == 1 and n_steps == 66200 > max(FIRST_SIZE, n_win // 64) == FIRST_SIZE and n_steps + 2 * n_tiles + 64 < n_win // 8
    names = write_inputs(tmp_path, cols)
    out, err = raft_twice(tmp_path, p.cli_args(), {})
    assert "derived by the engine" in err and "TIMING coverage_encoding delta4\n" in err and attempts_of(err) == 2, err
    check_against_oracle(tmp_path, "four-bit steps -> longer list", p, cols, names, out, want, p.cli_args())


@pytest.mark.parametrize("n_exc", [FIRST_SIZE - 1, FIRST_SIZE, FIRST_SIZE + 1])
def test_exactly_at_the_first_size(tmp_path, n_exc):
    """The byte case with 65,535, 65,536 and 65,537 windows at 256: the first two fit the list's first size and one attempt serves
    them; one more window and a second attempt runs (more than one window in 16: in two bytes)."""
    cols = byte_set([n_exc - n_exc // 2, n_exc // 2, 100, 100, 100])
    p = RaftParams(reso=1, est_cov=30)
    want = oracle_run(p, *cols)
    n_win = int(want["cov"].size)
    assert int((want["cov"] >= 255).sum()) == n_exc and max(FIRST_SIZE, n_win // 64) == FIRST_SIZE and n_exc > n_win // 16
    names = write_inputs(tmp_path, cols)
    out, err = raft_twice(tmp_path, ["-r", "1", "-e", "30"], {"RAFT_NO_DELTA4": "1"})
    second = n_exc > FIRST_SIZE
    assert f"TIMING coverage_encoding {'uint16' if second else 'uint8'}\n" in err and attempts_of(err) == (2 if second else 1), err
    check_against_oracle(tmp_path, f"{n_exc} windows on the list", p, cols, names, out, want, ["-r", "1", "-e", "30"])
