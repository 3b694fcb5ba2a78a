"""GPU: the pre-split job and its exchange at their structural edges (raft_hip_run_presplit_local, raft_hip_presplit_symmetric[_local],
raft_hip_group_sides, raft_hip_exchange[_local]; the sets are tests/presplit_cases.py's, kept honest by tests/test_presplit_cases.py).

Fewer records than ranks, ranks that own no reads, slices without records, ranks that receive nothing, sixteen and seventeen runs at
one rank, contexts that held a larger job before -- everything against the oracle on the whole set, everything exact.  One process,
ranks as contexts of the one GPU; the RCCL forms with the one rank this box can hold."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from presplit_cases import CASES, P30, Model, all_vs_all, by_name, case_id, record_cut
from raft_testlib import GOLDEN, ROOT, RaftParams, assert_same_result, md5, oracle_run, result_from_ref_files
from test_gpu_exchange import rank_slice_of

pytestmark = pytest.mark.gpu

SMALL = [c for c in CASES if c.world <= 8]
WIDE = [c for c in CASES if c.world > 8]
LIMIT = {1: 255, 2: 65535}
RESULT_KEYS = ("cov_offset", "rep_offset", "rep_s", "rep_e", "frag_offset", "frag_begin", "frag_end")


@pytest.fixture(scope="module")
def engs():
    """Eight contexts that every test of this file shares: whatever a job leaves in them meets the next one."""
    from raft_amd import engine
    es = [engine.Engine(P30, device=0) for _ in range(8)]
    yield es
    for e in es:
        e.close()


def check_rank(torch, eng, p, got, read_len, b0, b1, want, what):
    """The grouped pass of one rank over what it received equals the oracle's outputs for the rank's reads (the rank may own no
    reads and may have received nothing)."""
    rl = read_len[b0:b1]
    d_rl = torch.as_tensor(np.ascontiguousarray(rl)).to("cuda:0")
    B = int(((rl.astype(np.int64) + p.reso - 1) // p.reso).sum())
    if got["qe"] is None:
        eng.run_device_windows(d_rl, got["rec_offset"], got["qs"], n_bins=B)
    else:
        eng.run_device_grouped(d_rl, got["rec_offset"], None, got["qs"], got["qe"], n_bins=B)
    s = eng.finish()
    res = eng.fetch()
    exp = rank_slice_of(want, b0, b1)
    for k in exp:
        assert np.array_equal(res[k], exp[k]), (what, k)
    assert s.interval_path == 0 and s.n_intervals == got["n_rec"] and s.n_reads == b1 - b0, what
    if got["n_rec"]:
        assert s.n_segments == got["n_runs"], what
    return s


class Job:
    """Columns, ranks and the oracle's outputs of one pre-split job."""

    def __init__(self, name, world, p, read_len, cols):
        self.name, self.world, self.p = name, world, p
        self.read_len, self.cols = np.ascontiguousarray(read_len, np.int32), [np.ascontiguousarray(c, np.int32) for c in cols]
        self.want = oracle_run(p, self.read_len, *self.cols)

    @classmethod
    def of(cls, case):
        j = cls.__new__(cls)
        j.name, j.world, j.p, j.read_len, j.cols, j.want = case.name, case.world, case.p, case.read_len, case.cols, case.oracle()
        return j


_LARGER = {}


def larger_job(world):
    """A job larger than every case (24 reads, 552 intervals), to run BEFORE a case on the same contexts: one record per pair, not
    symmetric, every rank busy -- on 64 ranks both records per pair, sorted (a read's records lie in three or four slices: the sides
    of unsorted pairs would arrive from more than 16 slices, which is more runs than a rank takes)."""
    if world not in _LARGER:
        lens = [3000] * 24
        recs = np.asarray(all_vs_all(lens, half=world <= 8), np.int32)
        _LARGER[world] = Job(f"larger/w{world}", world, P30, lens, [recs[:, k] for k in range(6)])
    return _LARGER[world]


def run_job(es, job, width=1, out=None):
    for e in es[:job.world]:
        e.set_params(job.p)
    if out is None:
        out = es[0].host_output_buffers(job.read_len, pinned=False, width=width)
    return es[0].run_presplit(job.read_len, *job.cols, others=es[1:job.world], out=out)


def assert_job(res, s, job, width, what):
    want = job.want
    cov = res["cov8"].astype(np.int32)
    assert np.all(np.diff(res["exc_index"]) > 0), what
    assert np.array_equal(res["exc_index"], np.flatnonzero(want["cov"] >= LIMIT[width])), (what, res["exc_index"])
    cov[res["exc_index"]] = res["exc_value"]
    assert np.array_equal(cov, want["cov"]), (what, "cov")
    for k in RESULT_KEYS:
        assert np.array_equal(res[k], want[k]), (what, k, res[k], want[k])
    assert (s.symmetric, s.high_cov, s.n_records, s.n_devices_used, s.n_reads) == \
        (want["symmetric"], want["high_cov"], job.cols[0].size, job.world, job.read_len.size), what
    for k in ("total_coverage", "total_windows", "total_repeat_length", "total_read_length", "n_intervals"):
        assert getattr(s, k) == want[k], (what, k)
    assert (s.n_fragments, s.n_repeats, s.n_bins) == (want["frag_begin"].size, want["rep_s"].size, want["cov"].size), what


def check_job(es, job, width=1, what=""):
    res, s = run_job(es, job, width)
    assert_job(res, s, job, width, f"{job.name} width {width} {what}")


def job_sequence(es, case):
    """Twice on the same contexts, and once more after a larger job has been through them."""
    from raft_amd import engine
    job = Job.of(case)
    for width in case.widths:
        if width == 8:                                   # four-bit steps: chunks would have to begin on multiples of four windows
            with pytest.raises(engine.RaftError) as e:
                run_job(es, job, out=es[0].host_output_buffers(job.read_len, pinned=False, width=8))
            assert e.value.code == engine.ERR_PARAM
            continue
        check_job(es, job, width, "first")
        check_job(es, job, width, "again")
        check_job(es, larger_job(case.world), width, f"before {case.name}")
        check_job(es, job, width, "after a larger job")


# ---- 1. the whole job ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", SMALL, ids=case_id)
def test_job_equals_the_oracle(engs, case):
    job_sequence(engs, case)


def test_job_on_64_ranks_equals_the_oracle():
    from raft_amd import engine
    es = [engine.Engine(P30, device=0) for _ in range(64)]
    assert WIDE and all(c.world == 64 for c in WIDE)
    for case in WIDE:
        job_sequence(es, case)
    for e in es:
        e.close()


# ---- 2. capacities across ranks -----------------------------------------------------------------------------------------------

def test_capacities_are_the_sum_over_the_ranks(engs):
    """deep_windows/w4: two of the four exceptions, one of the two repeats and six of the 27 fragments are the LAST rank's -- a
    capacity one short of the total is exceeded by a rank other than the first."""
    from raft_amd import engine
    case = by_name("deep_windows/w4")
    job, want = Job.of(case), case.oracle()
    m = Model(case)
    n_exc, n_rep, n_frag = int((want["cov"] >= 255).sum()), want["rep_s"].size, want["frag_begin"].size
    last = m.bounds[3]                                   # rank 3's first read
    assert int((want["cov"][m.prefix[last]:] >= 255).sum()) >= 1 and (want["cov"][:m.prefix[m.bounds[1]]] < 255).all()
    assert want["rep_offset"][-1] > want["rep_offset"][last] > 0 and want["frag_offset"][-1] > want["frag_offset"][last] > 0

    def buffers(exc=None, rep=None, frag=None):
        engs[0].set_params(job.p)                        # (the buffers' sizes follow the parameters)
        out = engs[0].host_output_buffers(job.read_len, pinned=False, exc_cap=exc if exc is not None else 64)
        for keys, n in ((("rep_s", "rep_e"), rep), (("frag_begin", "frag_end"), frag)):
            if n is not None:
                for k in keys:
                    out[k] = out[k][:n]
        return out
    with pytest.raises(engine.RaftError) as e:
        run_job(engs, job, out=buffers(exc=n_exc - 1))
    assert e.value.code == engine.ERR_TOO_LARGE and engs[0].last_n_exc == n_exc
    res, s = run_job(engs, job, out=buffers(exc=n_exc))
    assert engs[0].last_n_exc == n_exc
    assert_job(res, s, job, 1, "exc_cap exact")
    for short, exact in ((dict(rep=n_rep - 1), dict(rep=n_rep)), (dict(frag=n_frag - 1), dict(frag=n_frag))):
        with pytest.raises(engine.RaftError) as e:
            run_job(engs, job, out=buffers(**short))
        assert e.value.code == engine.ERR_TOO_LARGE, short
        res, s = run_job(engs, job, out=buffers(**exact))
        assert_job(res, s, job, 1, f"{exact} exact")


# ---- 3. errors ----------------------------------------------------------------------------------------------------------------

def test_errors_name_their_record_and_leave_the_contexts_usable(engs):
    from raft_amd import engine
    good = by_name("four_records/w3")
    job = Job.of(good)
    for e in engs[:3]:
        e.set_params(good.p)
    for column in (0, 3):                                # a query / a target outside [0, n_reads), in the last rank's slice
        cols = [c.copy() for c in job.cols]
        cols[column][-1] = 7
        index = {}
        for how in ("presplit", "multi"):
            with pytest.raises(engine.RaftError) as e:
                if how == "presplit":
                    engs[0].run_presplit(job.read_len, *cols, others=engs[1:3])
                else:
                    engs[0].run_pipelined(job.read_len, *cols, others=engs[1:3])
            assert e.value.code == engine.ERR_READ_ID, (column, how)
            index[how] = e.value.index
        print("error_index of a read id out of range, column", column, index)
        assert index == {"presplit": good.n_rec - 1, "multi": good.n_rec - 1}, (column, index)
        check_job(engs, job, what="after a read id out of range")
    rl = job.read_len.copy()
    rl[1] = -5
    with pytest.raises(engine.RaftError) as e:
        engs[0].run_presplit(rl, *job.cols, others=engs[1:3])
    assert e.value.code == engine.ERR_PARAM and e.value.index == 1
    check_job(engs, job, what="after a negative length")
    with pytest.raises(engine.RaftError) as e:           # 65 ranks (the same context 65 times: the count is refused before any is used)
        engs[0].run_presplit(job.read_len, *job.cols, others=[engs[1]] * 64)
    assert e.value.code == engine.ERR_PARAM
    check_job(engs, job, what="after 65 ranks")


# ---- 4. raft_hip_exchange_local on hand-built slices --------------------------------------------------------------------------

N_READS = 8
LENS = np.full(N_READS, 1000, np.int32)


def hand_slice(rank, runs):
    """A slice of `runs` = per run the read ids of its records (ascending): offsets [n_runs, N_READS + 1], qs, qe, and the ids."""
    off = np.zeros((len(runs), N_READS + 1), np.int64)
    ids, at = [], 0
    for j, reads in enumerate(runs):
        reads = np.asarray(reads, np.int64)
        assert np.all(np.diff(reads) >= 0)
        off[j] = at + np.searchsorted(reads, np.arange(N_READS + 1))
        ids.append(reads)
        at += reads.size
    ids = np.concatenate(ids).astype(np.int32) if ids else np.empty(0, np.int32)
    k = np.arange(ids.size)
    qs = ((rank * 97 + k * 31 + ids * 13) % 400).astype(np.int32)
    qe = (qs + 100 + (rank * 7 + k * 11) % 500).astype(np.int32)
    return off, qs, qe, ids


def device_slices(parts, windows=False, device_offsets=False):
    import torch
    from raft_amd import engine, hostio
    out = []
    for off, qs, qe, _ in parts:
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to("cuda:0")
        if windows and not qs.size:
            out.append(engine.Slice(off, t(qs), device_offsets=device_offsets))
        elif windows:
            out.append(engine.Slice(off, t(hostio.pack_windows(qs, qe, 50).view(np.int32)), device_offsets=device_offsets))
        else:
            out.append(engine.Slice(off, t(qs), t(qe), device_offsets=device_offsets))
    return out


def oracle_of(parts):
    ids = np.concatenate([p[3] for p in parts])
    qs, qe = np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts])
    return oracle_run(P30, LENS, ids, qs, qe, ids, qs, qe)


def exchange_and_check(es, bounds, parts, runs_expected, windows=False, what=""):
    import torch
    from raft_amd import engine
    world = len(parts)
    for e in es[:world]:
        e.set_params(RaftParams(est_cov=30, symmetric_mode=1))
    want = oracle_of(parts)
    got = engine.exchange_local(es[:world], np.asarray(bounds, np.int64), device_slices(parts, windows))
    assert [g["n_runs"] for g in got] == [max(r, 1) for r in runs_expected], what
    assert sum(g["n_rec"] for g in got) == sum(p[3].size for p in parts)
    for g in range(world):
        if got[g]["n_rec"]:
            assert (got[g]["qe"] is None) == windows, (what, g)       # the form of what arrives is the form of what was sent
        check_rank(torch, es[g], P30, got[g], LENS, int(bounds[g]), int(bounds[g + 1]), want, f"{what} rank {g}")
    return got


ALL = list(range(N_READS))


def test_exchange_local_sixteen_runs_arrive_seventeen_do_not(engs):
    from raft_amd import engine
    bounds4, bounds5 = [0, 2, 4, 6, 8], [0, 2, 4, 6, 8, 8]
    four = [hand_slice(r, [ALL] * 4) for r in range(4)]
    exchange_and_check(engs, bounds4, four, [16] * 4, what="4 ranks x 4 runs")
    # a run without records for a destination is not a run there: rank 3's last run has nothing on reads 0 and 1
    fifteen = four[:3] + [hand_slice(3, [ALL] * 3 + [ALL[2:]])]
    exchange_and_check(engs, bounds4, fifteen, [15, 16, 16, 16], what="15 runs at rank 0")
    # ... nor are the four runs of a fifth rank whose slice is empty
    empty = hand_slice(4, [[]] * 4)
    exchange_and_check(engs, bounds5, four + [empty], [16] * 4 + [0], what="a fifth rank without records")
    # seventeen runs at rank 0 (the first rank looked at): 5 x 4 with three of the fifth rank's pieces for it emptied, or one single
    # record of the fifth rank on read 0
    for fifth in ([ALL, ALL[2:], ALL[2:], ALL[2:]], [[0], [], [], []]):
        with pytest.raises(engine.RaftError) as e:
            engine.exchange_local(engs[:5], np.asarray(bounds5, np.int64), device_slices(four + [hand_slice(4, fifth)]))
        assert e.value.code == engine.ERR_TOO_LARGE and "more than 16 runs arrive at one rank" in str(e.value)
    exchange_and_check(engs, bounds4, four, [16] * 4, what="after seventeen runs")


@pytest.mark.parametrize("windows", [False, True], ids=["coordinates", "windows"])
def test_exchange_local_takes_its_form_from_the_first_slice_with_records(engs, windows):
    from raft_amd import engine
    bounds = [0, 3, 5, 8]
    parts = [hand_slice(0, [[]]), hand_slice(1, [ALL, ALL[1:]]), hand_slice(2, [[0, 0, 4, 7]])]
    got = exchange_and_check(engs, bounds, parts, [3, 3, 3], windows, what="rank 0's slice empty")
    assert all((g["qe"] is None) == windows for g in got)
    # no records anywhere: the coordinate form
    got = exchange_and_check(engs, bounds, [hand_slice(r, [[]]) for r in range(3)], [0, 0, 0], False, what="no records")
    assert all(g["qe"] is not None and g["n_rec"] == 0 for g in got)
    # a genuine mix is the caller's error, whichever of the two comes first
    a, b = device_slices(parts[1:2], windows)[0], device_slices(parts[2:3], not windows)[0]
    nothing = device_slices(parts[:1])[0]
    for sl in ([nothing, a, b], [a, nothing, b], [b, a, nothing]):
        with pytest.raises(engine.RaftError) as e:
            engine.exchange_local(engs[:3], np.asarray(bounds, np.int64), sl)
        assert e.value.code == engine.ERR_PARAM
    exchange_and_check(engs, bounds, parts, [3, 3, 3], windows, what="after a mix")


def test_exchange_local_refuses_offsets_and_bounds_that_do_not_fit(engs):
    import torch
    from raft_amd import engine
    bounds = np.array([0, 3, 5, 8], np.int64)
    parts = [hand_slice(r, [ALL, ALL]) for r in range(3)]

    def refused(bounds, parts):
        with pytest.raises(engine.RaftError) as e:
            engine.exchange_local(engs[:3], bounds, device_slices(parts))
        assert e.value.code == engine.ERR_PARAM

    def with_offsets(change):
        off = parts[1][0].copy()
        change(off)
        return [parts[0], (off,) + parts[1][1:], parts[2]]
    refused(bounds, with_offsets(lambda off: off.__setitem__((1, N_READS), 17)))          # past the slice's 16 records
    refused(bounds, with_offsets(lambda off: off.__setitem__((0, 0), -1)))                # before it
    refused(bounds, with_offsets(lambda off: off.__setitem__((0, 5), off[0, 3] - 1)))     # a step back between two bounds
    for bad in ([1, 3, 5, 8], [0, 3, 5, 7], [0, 5, 3, 8], [0, 3, 5, 9], [-1, 3, 5, 8]):
        refused(np.array(bad, np.int64), parts)
    exchange_and_check(engs, bounds, parts, [6, 6, 6], what="after refused arguments")
    # records without both coordinate columns never reach a kernel: the grouped pass refuses them on the host
    off, qs, qe, ids = hand_slice(0, [ALL])
    t = lambda a: torch.as_tensor(a).to("cuda:0")
    engs[0].set_params(RaftParams(est_cov=30, symmetric_mode=1))
    for hint in (-1, 160):
        with pytest.raises(engine.RaftError) as e:
            engs[0].run_device_grouped(t(LENS), t(off), None, t(qs), None, n_bins=hint)
        assert e.value.code == engine.ERR_PARAM and "records without both coordinate columns" in str(e.value)
    engs[0].run_device_grouped(t(LENS), t(off), None, t(qs), t(qe), n_bins=160)
    s = engs[0].finish()
    got = engs[0].fetch()
    got.update({k: getattr(s, k) for k in ("symmetric", "high_cov", "total_coverage", "total_windows", "total_repeat_length", "total_read_length")})
    want = oracle_of([(off, qs, qe, ids)])
    want["symmetric"] = 1
    assert_same_result(got, want, "after a refused pass")


# ---- 5. raft_hip_group_sides --------------------------------------------------------------------------------------------------

def assert_sides(sl, n_reads, cols, symmetric):
    """Read by read, the intervals of the slice are the sides the records have there (in any order)."""
    from raft_testlib import sides_reference
    off, start, end = sides_reference(n_reads, *cols, symmetric)
    assert sl.off.shape == (1, n_reads + 1) and np.array_equal(sl.off[0], off) and sl.qs.numel() == sl.qe.numel() == off[-1]
    qs, qe = sl.qs.cpu().numpy(), sl.qe.cpu().numpy()
    for r in range(n_reads):
        a, b = int(off[r]), int(off[r + 1])
        assert sorted(zip(qs[a:b].tolist(), qe[a:b].tolist())) == sorted(zip(start[a:b].tolist(), end[a:b].tolist())), r


def test_group_sides_edges():
    import torch
    from raft_amd import engine
    fresh = engine.Engine(P30, device=0)                 # a context that has grouped nothing yet
    empty = [torch.empty(0, dtype=torch.int32, device="cuda:0")] * 6
    for symmetric in (False, True):
        sl0 = fresh.group_sides(5, *empty, symmetric=symmetric)
        assert sl0.qs.numel() == 0 and sl0.qe.numel() == 0 and sl0.off.shape == (1, 6) and not sl0.off.any()
        c = sl0.c()
        assert sl0.ptrs[0] and sl0.ptrs[1] and c.d_qs and c.d_qe and c.n_rec == 0 and c.n_runs == 1    # coordinate form, said by an empty slice too
    rng = np.random.default_rng(3)
    n_reads, n = 9, 40
    dev = lambda cols: [torch.as_tensor(np.ascontiguousarray(c, np.int32)).to("cuda:0") for c in cols]
    coords = lambda: [rng.integers(0, 500, n).astype(np.int32) for _ in range(2)]
    qs, ts = coords()
    for name, qid, tid in (("self-overlaps", rng.integers(0, n_reads, n), None), ("one read", np.full(n, 4), np.full(n, 4)),
                           ("first and last read", rng.choice([0, n_reads - 1], n), rng.choice([0, n_reads - 1], n)),
                           ("all onto one read", rng.integers(0, n_reads, n), np.full(n, 2))):
        tid = qid if tid is None else tid
        cols = [qid.astype(np.int32), qs, qs + 100, tid.astype(np.int32), ts, ts + 50]
        for symmetric in (False, True):
            sl = fresh.group_sides(n_reads, *dev(cols), symmetric=symmetric)
            assert_sides(sl, n_reads, cols, symmetric)
            if name in ("self-overlaps", "one read"):
                assert sl.qs.numel() == n, name              # a self-overlap has ONE side, symmetric or not
        sl0 = fresh.group_sides(n_reads, *empty, symmetric=False)    # ... and nothing again, after something
        assert sl0.qs.numel() == 0 and not sl0.off.any() and sl0.ptrs[0] and sl0.ptrs[1]
    fresh.close()


# ---- 6. raft_hip_presplit_symmetric_local -------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [c for c in SMALL if c.n_rec or c.name == "no_records/w3"], ids=case_id)
def test_flag_of_every_case(engs, case):
    import torch
    from raft_amd import engine
    cut = record_cut(case.n_rec, case.world)
    cols = [torch.as_tensor(c).to("cuda:0") for c in case.cols]
    parts = [[c[cut[r]:cut[r + 1]].contiguous() for c in cols] for r in range(case.world)]
    for _ in range(2):
        assert engine.presplit_symmetric_local(engs[:case.world], parts) is bool(case.symmetric)
    if case.symmetric and case.n_rec == 2:               # the pair the other way round: the first record is rank-wise the later one
        assert engine.presplit_symmetric_local(engs[:case.world], parts[::-1]) is True


GRID = 256 * 256 * 16                                    # records one sweep of mirror_search_kernel's grid covers


@pytest.mark.parametrize("at", [GRID - 1, GRID, GRID + 299, None], ids=["last of the grid", "first of the stride", "last record", "nowhere"])
def test_flag_beyond_one_sweep_of_the_grid(engs, at):
    """GRID + 300 records on one rank: the threads of the first 300 lanes take a second record.  Query ids are below 1000 and target
    ids from 1000 up, so nothing mirrors record 0 but the record put there."""
    import torch
    from raft_amd import engine
    n = GRID + 300
    rng = np.random.default_rng(11)
    cols = [rng.integers(0, 1000, n).astype(np.int32), rng.integers(0, 5000, n).astype(np.int32), rng.integers(5000, 9000, n).astype(np.int32),
            rng.integers(1000, 2000, n).astype(np.int32), rng.integers(0, 5000, n).astype(np.int32), rng.integers(5000, 9000, n).astype(np.int32)]
    if at is not None:
        for k, j in enumerate((3, 4, 5, 0, 1, 2)):
            cols[k][at] = cols[j][0]
    m = np.ones(n, bool)
    for k, j in enumerate((3, 4, 5, 0, 1, 2)):
        m &= cols[k] == cols[j][0]
    m[0] = False
    assert np.flatnonzero(m).tolist() == ([at] if at is not None else [])
    dcols = [torch.as_tensor(c).to("cuda:0") for c in cols]
    assert engine.presplit_symmetric_local(engs[:1], [dcols]) is (at is not None)
    # ... and with the stream on two ranks, cut inside the second sweep
    cut = GRID + 150
    parts = [[c[:cut].contiguous() for c in dcols], [c[cut:].contiguous() for c in dcols]]
    assert engine.presplit_symmetric_local(engs[:2], parts) is (at is not None)


# ---- 7. the one-rank RCCL communicator ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def comm():
    from raft_amd import engine
    c = engine.Comm(0, engine.Comm.unique_id(), 0, 1)
    yield c
    c.close()


def rebased(off):
    """What one rank receives from itself: the runs with records, each counting from where the one before ended."""
    keep = [r for r in off if r[-1] > r[0]]
    if not keep:
        return np.zeros((1, off.shape[1]), np.int64)
    out, base = [], 0
    for r in keep:
        out.append(base + r - r[0])
        base += r[-1] - r[0]
    return np.asarray(out, np.int64)


def comm_exchange_and_check(comm, eng, n_reads, runs, device_offsets, what):
    import torch
    from raft_amd import engine
    eng.set_params(RaftParams(est_cov=30, symmetric_mode=1))
    rng = np.random.default_rng(n_reads * 31 + len(runs))
    lens = np.full(n_reads, 500, np.int32)
    off = np.zeros((len(runs), n_reads + 1), np.int64)
    ids, at = [], 0
    for j, reads in enumerate(runs):
        reads = np.sort(np.asarray(reads, np.int64))
        off[j] = at + np.searchsorted(reads, np.arange(n_reads + 1))
        ids.append(reads)
        at += reads.size
    ids = np.concatenate(ids).astype(np.int32) if at else np.empty(0, np.int32)
    qs = rng.integers(0, 250, ids.size).astype(np.int32)
    qe = (qs + rng.integers(1, 250, ids.size)).astype(np.int32)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to("cuda:0")
    sl = engine.Slice(off, t(qs), t(qe), device_offsets=device_offsets)
    if not at:                                           # an empty slice of a coordinate-form exchange still says so (include/raft_hip.h)
        keep = t(np.zeros(1, np.int32))
        sl.ptrs = (keep.data_ptr(), keep.data_ptr())
    want = oracle_run(P30, lens, ids, qs, qe, ids, qs, qe)
    for rep in range(2):
        got = comm.exchange(eng, np.array([0, n_reads], np.int64), sl)
        exp = rebased(off)
        assert (got["n_reads"], got["n_rec"], got["n_runs"]) == (n_reads, ids.size, exp.shape[0]), what
        assert np.array_equal(got["rec_offset"].cpu().numpy(), exp), what
        keep_runs = [j for j in range(len(runs)) if off[j, -1] > off[j, 0]]
        sent = np.concatenate([np.arange(off[j, 0], off[j, -1]) for j in keep_runs]) if keep_runs else np.empty(0, np.int64)
        assert got["qe"] is not None and np.array_equal(got["qs"].cpu().numpy(), qs[sent]) and np.array_equal(got["qe"].cpu().numpy(), qe[sent]), what
        check_rank(torch, eng, P30, got, lens, 0, n_reads, want, f"{what} pass {rep}")


@pytest.mark.parametrize("device_offsets", [False, True], ids=["offsets uploaded", "offsets on the device"])
def test_comm_one_rank_edges(engs, comm, device_offsets):
    import torch
    eng = engs[0]
    every = lambda n: list(range(n))
    comm_exchange_and_check(comm, eng, 84, [every(84), [3, 3, 80], every(84)], device_offsets, "(84 + 1) * 3 = 255")
    comm_exchange_and_check(comm, eng, 5, [[]], device_offsets, "an empty slice after a larger one")
    comm_exchange_and_check(comm, eng, 0, [[]], device_offsets, "no reads at all")
    comm_exchange_and_check(comm, eng, 63, [every(63), [0], [62], every(63)[::2]], device_offsets, "four runs to itself: (63 + 1) * 4 = 256")
    comm_exchange_and_check(comm, eng, 63, [every(63), [], [62], []], device_offsets, "two of four runs without records")
    for n in (254, 255, 256):
        comm_exchange_and_check(comm, eng, n, [every(n)[1::3] + [n - 1, n - 1]], device_offsets, f"one run, {n + 1} offsets")
    empty = [torch.empty(0, dtype=torch.int32, device="cuda:0")] * 6
    assert comm.symmetric(eng, empty) is False
    case = by_name("mirrored_pair/w3")
    assert comm.symmetric(eng, [torch.as_tensor(c).to("cuda:0") for c in case.cols]) is True
    assert comm.symmetric(eng, [torch.as_tensor(c[:1].copy()).to("cuda:0") for c in case.cols]) is False


# ---- 8. the command line ------------------------------------------------------------------------------------------------------

RAFT = os.path.join(ROOT, "raft_amd", "bin", "raft")


@pytest.mark.parametrize("ranks", [3, 8])
@pytest.mark.parametrize("name", ["g6_mirrored_pair", "g7_half_pair"])
def test_cli_fewer_records_than_ranks(tmp_path, name, ranks):
    """RAFT_RANKS=3 / 8 on two reads and two records (one overlap and its mirror) or one (the mirror dropped): the four files and stdout
    are the run's without RAFT_RANKS, the reference's (tests/golden/micro), and their arrays the oracle's."""
    from test_gpu_cli import strip_timing
    from test_oracle_golden import MAN, _micro_columns, _params_from_args
    d = os.path.join(GOLDEN, "micro", name)
    meta = MAN["micro"][name]
    outs = {}
    for how, env in (("one", {}), ("ranks", {"RAFT_RANKS": str(ranks)})):
        w = tmp_path / how
        w.mkdir()
        shutil.copy(os.path.join(d, "reads.fa"), w)
        shutil.copy(os.path.join(d, "overlaps.paf"), w)
        r = subprocess.run([RAFT] + meta["args"] + ["reads.fa", "overlaps.paf"], cwd=w, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120,
                           env=dict(os.environ, RAFT_TIMING="1", **env))
        assert r.returncode == 0, r.stdout.decode() + r.stderr.decode()
        files = sorted(f for f in os.listdir(w) if f not in ("reads.fa", "overlaps.paf"))
        assert files == meta["outputs"], (how, files)
        outs[how] = (strip_timing(r.stdout.decode()), {f: open(w / f, "rb").read() for f in files})
        used = [l for l in r.stderr.decode().splitlines() if l.startswith("TIMING devices_used")]
        assert how == "one" or (used and used[0].split()[2] == str(ranks) and "pre-split" in used[0]), r.stderr.decode()
    assert outs["ranks"] == outs["one"]
    assert outs["ranks"][0] == open(os.path.join(d, "expect.stdout")).read()
    for f, data in outs["ranks"][1].items():
        assert md5(data) == md5(open(os.path.join(d, "expect." + f), "rb").read()), (name, f)
    names, lens, cols = _micro_columns(d)
    want = oracle_run(_params_from_args(meta["args"]), lens, *cols)
    assert want["symmetric"] == (1 if name == "g6_mirrored_pair" else 0)
    got = result_from_ref_files(str(tmp_path / "ranks" / "raft"), names)
    for k, v in got.items():
        assert np.array_equal(v, want[k]), (name, ranks, k)
