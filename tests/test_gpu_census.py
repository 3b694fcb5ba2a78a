"""GPU: raft_hip_census_device / raft_hip_census_host (raft_amd/csrc/census.hpp) -- intervals per read and contained flags from a record
stream -- exact against numpy on the input columns: np.bincount for the counts, boolean masks and np.logical_or.at for the flags."""
import os
import re

import numpy as np
import pytest
from raft_testlib import ROOT, runs_of

from raft_amd.params import RaftParams

pytestmark = pytest.mark.gpu


def launch_constants():
    text = open(os.path.join(ROOT, "raft_amd", "csrc", "record_stream.hpp")).read()
    k = {name: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1)) for name in ("kStreamThreads", "kStreamLaneRecords", "kStreamMaxBlocks")}
    return k["kStreamThreads"], k["kStreamLaneRecords"], k["kStreamMaxBlocks"]


def want_census(rl, qid, qs, qe, tid, ts, te, symmetric):
    n = rl.size
    rl64 = rl.astype(np.int64)
    intervals = np.bincount(qid, minlength=n).astype(np.int64)
    flags = np.zeros(n, np.uint8)
    q_side = np.zeros(n, bool)
    np.logical_or.at(q_side, qid, (qs == 0) & (qe == rl64[qid]) & (rl64[tid] > rl64[qid]))
    flags[q_side] |= 1
    if not symmetric:
        intervals += np.bincount(tid[tid != qid], minlength=n)
        t_side = np.zeros(n, bool)
        np.logical_or.at(t_side, tid, (ts == 0) & (te == rl64[tid]) & (rl64[qid] > rl64[tid]))
        flags[t_side] |= 2
    return intervals, flags


def check(eng, cols, symmetric, what, forms=("host", "device")):
    import torch
    rl, qid, qs, qe, tid, ts, te = cols
    wi, wf = want_census(*cols, symmetric)
    out = None
    for form in forms:
        c = cols if form == "host" else [torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0") for x in cols]
        got = eng.census(c[0], c[1], c[2], c[3], c[4], None if symmetric else c[5], None if symmetric else c[6], symmetric=symmetric)
        assert got["intervals"].dtype == np.int32 and got["contained"].dtype == np.uint8
        bad = np.flatnonzero(got["intervals"] != wi)
        assert bad.size == 0, f"{what} ({form}, symmetric={symmetric}): intervals differ on {bad.size} reads, first {bad[0]}: got {got['intervals'][bad[0]]} want {wi[bad[0]]}"
        bad = np.flatnonzero(got["contained"] != wf)
        assert bad.size == 0, f"{what} ({form}, symmetric={symmetric}): flags differ on {bad.size} reads, first {bad[0]}: got {got['contained'][bad[0]]} want {wf[bad[0]]}"
        assert got["n_contained"] == int((wf != 0).sum()), (what, form)
        assert eng.last_census_seconds >= 0.0
        if out is not None:                                # device tensors and host arrays give the same result
            assert np.array_equal(out["intervals"], got["intervals"]) and np.array_equal(out["contained"], got["contained"])
        out = got
    return out


@pytest.fixture(scope="module")
def eng():
    from raft_amd import engine
    e = engine.Engine(RaftParams(est_cov=3), device=0)
    yield e
    e.close()


def records(rl, qid, tid, seed, full_fraction=0.3):
    """Coordinates for the given pairs: a share of the sides cover their read from end to end, some miss by one base at either end."""
    rng = np.random.default_rng(seed)
    n = qid.size

    def side(ids):
        L = rl[ids].astype(np.int64)
        s = (rng.random(n) * L * 0.5).astype(np.int64)
        e = np.minimum(L, s + 1 + (rng.random(n) * L).astype(np.int64))
        kind = rng.random(n)
        full = kind < full_fraction
        s[full] = 0; e[full] = L[full]
        short = (kind >= full_fraction) & (kind < full_fraction + 0.1)      # qs == 0 with qe == len - 1
        s[short] = 0; e[short] = np.maximum(L[short] - 1, 0)
        late = (kind >= full_fraction + 0.1) & (kind < full_fraction + 0.2)  # qs == 1 with qe == len
        s[late] = np.minimum(1, L[late]); e[late] = L[late]
        return s.astype(np.int32), e.astype(np.int32)
    qs, qe = side(qid)
    ts, te = side(tid)
    return [rl, qid.astype(np.int32), qs, qe, tid.astype(np.int32), ts, te]


# ---- containment ------------------------------------------------------------------------------------------------------------------------

def test_containment_rules(eng):
    rl = np.array([1000, 2000, 1000, 500, 3000, 0], np.int32)
    rows = [
        # qid qs  qe    tid ts te
        (0, 0, 999, 1, 0, 2000),      # qs == 0 with qe == len - 1: not contained; the target side covers read 1, but read 0 is shorter
        (0, 1, 1000, 1, 5, 900),      # qs == 1 with qe == len: not contained
        (0, 0, 1000, 2, 0, 1000),     # equal lengths: neither
        (1, 0, 2000, 0, 3, 800),      # container shorter: not contained
        (3, 0, 500, 3, 0, 500),       # a self overlap: counted once, never contained
        (3, 0, 500, 4, 7, 400),       # read 3 contained through its query side only
        (4, 10, 900, 2, 0, 1000),     # read 2 contained through its target side only
        (3, 0, 500, 4, 100, 700),     # the same pair again
        (2, 0, 1000, 1, 100, 1100),   # read 2 through its query side as well: both bits
        (5, 0, 0, 0, 10, 20),         # a read of length 0 lies inside anything longer
    ]
    cols = [rl] + [np.array([r[k] for r in rows], np.int32) for k in range(6)]
    got = check(eng, cols, False, "rules")
    assert list(got["contained"]) == [0, 0, 3, 1, 0, 1] and got["n_contained"] == 3
    assert list(got["intervals"]) == [3 + 2, 1 + 3, 1 + 2, 3, 1 + 2, 1]
    got = check(eng, cols, True, "rules")
    assert list(got["contained"]) == [0, 0, 1, 1, 0, 1]
    assert list(got["intervals"]) == [3, 1, 1, 3, 1, 1]


def test_a_missing_target_column(eng):
    from raft_amd import engine
    rl = np.array([100, 200], np.int32)
    c = np.zeros(3, np.int32)
    for symmetric in (True, False):
        with pytest.raises(engine.RaftError) as e:
            eng.census(rl, c, c, c, None, None if symmetric else c, None if symmetric else c, symmetric=symmetric)
        assert e.value.code == engine.ERR_PARAM


# ---- stream shapes ----------------------------------------------------------------------------------------------------------------------

def sizes():
    threads, lane_records, _ = launch_constants()
    step = threads * lane_records                          # records one workgroup takes per step
    return [0, 1, 3, 4, 5, step - 1, step, step + 1]


def stream(shape, n_rec, n_reads, seed):
    rng = np.random.default_rng(seed)
    if shape == "sorted":
        qid = np.sort(rng.integers(0, n_reads, n_rec))
    elif shape == "two_runs":
        qid = np.concatenate([np.sort(rng.integers(0, n_reads, n_rec // 2)), np.sort(rng.integers(0, n_reads, n_rec - n_rec // 2))])
    elif shape == "shuffled":
        qid = rng.integers(0, n_reads, n_rec)
    elif shape == "alternating":
        qid = np.where(np.arange(n_rec) % 2 == 0, 3, 11)
    else:
        raise ValueError(shape)
    tid = rng.integers(0, n_reads, n_rec)
    own = rng.random(n_rec) < 0.1                          # a tenth of the records are self overlaps
    tid[own] = qid[own]
    return qid, tid


@pytest.mark.parametrize("shape", ["sorted", "two_runs", "shuffled", "alternating"])
def test_stream_shapes(eng, shape):
    rng = np.random.default_rng(5)
    n_reads = 97
    rl = rng.integers(0, 5000, n_reads).astype(np.int32)
    rl[::13] = rl[1]                                       # equal lengths among the reads
    for n_rec in sizes():
        qid, tid = stream(shape, n_rec, n_reads, 100 + n_rec)
        cols = records(rl, qid, tid, 7 + n_rec)
        for symmetric in (False, True):
            check(eng, cols, symmetric, f"{shape}, n_rec {n_rec}")


def test_every_record_on_one_read(eng):
    rng = np.random.default_rng(9)
    n_reads, n_rec = 50, 40000
    rl = rng.integers(100, 5000, n_reads).astype(np.int32)
    qid = np.full(n_rec, 17)
    tid = rng.integers(0, n_reads, n_rec)
    cols = records(rl, qid, tid, 3)
    for symmetric in (False, True):
        got = check(eng, cols, symmetric, "one read")
        assert got["intervals"][17] >= n_rec
    cols = records(rl, tid, qid, 4)                        # ... and every target side on one read
    check(eng, cols, False, "one target read")


RUNS = [63, 64, 65, 257, 1, 2, 257, 65, 64, 63, 5, 257, 4, 4, 4, 3, 1, 1, 256, 1024, 7]


@pytest.mark.parametrize("lead", [0, 1, 3, 62, 255, 1024 - 1])
def test_runs_across_lane_wave_and_workgroup_edges(eng, lead):
    """Runs of 63 / 64 / 65 / 257 records on one read, begun at every kind of offset (the last: T - 1, T the records of a workgroup
    step), against a random target column and against the target column in runs as well."""
    threads, lane_records, _ = launch_constants()
    assert threads * lane_records == 1024
    rng = np.random.default_rng(lead)
    n_reads = 65
    rl = rng.integers(100, 5000, n_reads).astype(np.int32)
    rl[::7] = rl[3]                                        # equal lengths among the reads
    qid = runs_of(RUNS, first_id=2, lead=lead)
    assert qid.max() < n_reads
    for what, tid in (("runs, random targets", rng.integers(0, n_reads, qid.size)), ("runs on both sides", qid[::-1].copy())):
        cols = records(rl, qid, tid, 11 + lead)
        for symmetric in (False, True):
            check(eng, cols, symmetric, what)


def test_more_records_than_the_capped_grid_takes_in_one_step(eng):
    threads, lane_records, max_blocks = launch_constants()
    n_rec = threads * lane_records * max_blocks + 4099
    rng = np.random.default_rng(21)
    n_reads = 30000
    rl = rng.integers(100, 30000, n_reads).astype(np.int32)
    qid, tid = stream("two_runs", n_rec, n_reads, 5)
    cols = records(rl, qid, tid, 6)
    for symmetric in (False, True):
        check(eng, cols, symmetric, "grid stride", forms=("device",))


def test_unaligned_columns(eng):
    """Device columns that do not begin on 16 bytes take the 4-byte loads."""
    import torch
    rng = np.random.default_rng(2)
    n_reads, n_rec = 300, 5003
    rl = rng.integers(10, 5000, n_reads).astype(np.int32)
    qid, tid = stream("sorted", n_rec + 1, n_reads, 8)
    full = records(rl, qid, tid, 9)
    dev = [torch.from_numpy(full[0]).to("cuda:0")] + [torch.from_numpy(x).to("cuda:0")[1:] for x in full[1:]]
    assert dev[1].data_ptr() % 16 == 4
    wi, wf = want_census(rl, *[x[1:] for x in full[1:]], False)
    got = eng.census(*dev, symmetric=False)
    assert np.array_equal(got["intervals"], wi) and np.array_equal(got["contained"], wf)


# ---- errors and invariants --------------------------------------------------------------------------------------------------------------

def test_ids_out_of_range(eng):
    from raft_amd import engine
    rng = np.random.default_rng(4)
    n_reads, n_rec = 500, 9000
    rl = rng.integers(10, 5000, n_reads).astype(np.int32)
    qid, tid = stream("sorted", n_rec, n_reads, 1)
    cols = records(rl, qid, tid, 2)
    for column, at, value in ((1, 17, n_reads + 5), (1, 4321, -1), (4, 17, n_reads), (4, 8999, -7)):
        for symmetric in (False, True):
            bad = [c.copy() for c in cols]
            bad[column][at] = value
            if column == 1:
                bad[4][at + 100] = n_reads + 1            # a later record's target is bad as well: the first record is named
            with pytest.raises(engine.RaftError) as e:
                eng.census(*bad[:5], None if symmetric else bad[5], None if symmetric else bad[6], symmetric=symmetric)
            assert e.value.code == engine.ERR_READ_ID and e.value.index == at, (column, at, symmetric, e.value.code, e.value.index)
            check(eng, cols, symmetric, "after the error", forms=("host",))


@pytest.mark.parametrize("symmetric", [False, True])
def test_the_counts_add_up_to_the_pass(symmetric):
    from raft_amd import engine
    from raft_amd.synth import make_overlaps
    o = make_overlaps(1500, coverage=20, seed=3, symmetric=symmetric)
    cols = [c.numpy() for c in (o.read_len,) + o.columns()]
    eng = engine.Engine(RaftParams(est_cov=20), device=0)
    try:
        eng.run_host(*cols)
        s = eng.finish()
        assert s.symmetric == (1 if symmetric else 0)
        got = check(eng, cols, symmetric, "make_overlaps")
        assert int(got["intervals"].astype(np.int64).sum()) == s.n_intervals
        eng.run_host(*cols)                                # a census while a pass is in flight leaves the pass alone
        check(eng, cols, symmetric, "pass in flight", forms=("host",))
        s2 = eng.finish()
        assert s2.n_intervals == s.n_intervals and s2.total_coverage == s.total_coverage
    finally:
        eng.close()
