"""GPU: a pass built on what the context's previous pass found (round 6, engine.hip run_pass `speculate`).

raft_hip_run_device waits for the device once on its way -- sizes, sorted runs -- unless the context's last pass went the
sorted-run way over a stream of the same shape (counts, column addresses, parameters): then the pass is built on what that one
found and the device verifies it.  Whatever is in the buffers, the results are the oracle's (chop.hpp:133-322, repeat.hpp:28-171)."""
import numpy as np
import pytest
from raft_testlib import assert_same_result, oracle_run

from raft_amd.params import RaftParams

pytestmark = pytest.mark.gpu
SPECULATED = 2


def _set(seed, n_reads=3000, n=60000, two_runs=True):
    rng = np.random.default_rng(seed)
    rl = rng.integers(3000, 40000, n_reads).astype(np.int32)
    runs = []
    for k in range(2 if two_runs else 1):
        qid = np.sort(rng.integers(0, n_reads, n // 2)).astype(np.int32)
        a = (rng.random(qid.size) * rl[qid] * 0.8).astype(np.int32)
        b = np.minimum(rl[qid], a + 1 + (rng.random(qid.size) * rl[qid] * 0.3).astype(np.int32)).astype(np.int32)
        runs.append((qid, a, b))
    return rl, tuple(np.concatenate([r[i] for r in runs]) for i in range(3))


def _result(eng, s):
    got = eng.fetch()
    got.update(symmetric=s.symmetric, high_cov=s.high_cov, total_coverage=s.total_coverage, total_windows=s.total_windows,
               total_repeat_length=s.total_repeat_length, total_read_length=s.total_read_length)
    return got


def test_second_pass_over_the_same_buffers_speculates_and_equals_the_oracle():
    import torch
    from raft_amd import engine
    p = RaftParams(est_cov=8, symmetric_mode=1)
    rl, (qid, a, b) = _set(1)
    want = oracle_run(p, rl, qid, a, b, qid, a, b); want["symmetric"] = 1
    dev = [torch.from_numpy(x).to("cuda:0") for x in (rl, qid, a, b)]
    eng = engine.Engine(p, device=0)
    flags = []
    for it in range(4):
        eng.run_device(*dev)
        s = eng.finish()
        flags.append(s.flags & SPECULATED)
        assert_same_result(_result(eng, s), want, f"pass {it}")
    assert flags[0] == 0 and all(f == SPECULATED for f in flags[1:]), flags
    # other coordinates in the same buffers: what was assumed (windows, run ends) still holds, the records are read afresh
    rng = np.random.default_rng(5)
    a2 = (rng.random(qid.size) * rl[qid] * 0.5).astype(np.int32)
    b2 = np.minimum(rl[qid], a2 + 1 + (rng.random(qid.size) * rl[qid] * 0.5).astype(np.int32)).astype(np.int32)
    dev[2].copy_(torch.from_numpy(a2)); dev[3].copy_(torch.from_numpy(b2))
    want2 = oracle_run(p, rl, qid, a2, b2, qid, a2, b2); want2["symmetric"] = 1
    eng.run_device(*dev)
    s = eng.finish()
    assert s.flags & SPECULATED
    assert_same_result(_result(eng, s), want2, "other coordinates, same shape")
    eng.close()


@pytest.mark.parametrize("what", ["lengths", "same_windows", "run_ends", "unsorted", "bad_id"])
def test_a_stream_that_is_not_what_was_assumed_is_run_the_long_way(what):
    """Same counts, same addresses, other contents: the device refutes the assumption (other window count; other run ends; no
    sorted runs at all; an id out of range) and the result -- or the error -- is what a fresh context gives."""
    import torch
    from raft_amd import engine
    p = RaftParams(est_cov=8, symmetric_mode=1)
    rl, (qid, a, b) = _set(2)
    dev = [torch.from_numpy(x).to("cuda:0") for x in (rl, qid, a, b)]
    eng = engine.Engine(p, device=0)
    for _ in range(2):
        eng.run_device(*dev); s = eng.finish()
    assert s.flags & SPECULATED
    rng = np.random.default_rng(8)
    rl2, qid2, a2, b2 = rl.copy(), qid.copy(), a.copy(), b.copy()
    if what == "lengths":
        rl2 = rl + 50 * rng.integers(1, 4, rl.size).astype(np.int32)          # more windows per read, the records still fit
    elif what == "same_windows":
        # every read one base longer where that leaves its window count alone: the geometry the context holds would still be right for the
        # pileup, the fragments' would not (chop.hpp:209-223) -- the lengths themselves are compared, not what was derived from them
        rl2 = rl + ((rl % 50 > 0) & (rl % 50 < 49)).astype(np.int32)
        assert (rl2 != rl).any() and np.array_equal((rl2 + 49) // 50, (rl + 49) // 50)
    elif what == "run_ends":
        h = qid.size // 2                                                     # the second run begins 1000 records later
        q = np.concatenate([np.sort(qid[:h + 1000]), np.sort(qid[h + 1000:])]).astype(np.int32)
        qid2 = q
        a2 = (rng.random(q.size) * rl[q] * 0.5).astype(np.int32); b2 = np.minimum(rl[q], a2 + 100).astype(np.int32)
    elif what == "unsorted":
        perm = rng.permutation(qid.size)
        qid2, a2, b2 = qid[perm], a[perm], b[perm]
    else:
        qid2[qid.size // 3] = rl.size + 7
    for t, x in zip(dev, (rl2, qid2, a2, b2)):
        t.copy_(torch.from_numpy(np.ascontiguousarray(x)))
    if what == "bad_id":
        eng.run_device(*dev)
        with pytest.raises(engine.RaftError) as e:
            eng.finish()
        assert e.value.code == engine.ERR_READ_ID
    else:
        want = oracle_run(p, rl2, qid2, a2, b2, qid2, a2, b2); want["symmetric"] = 1
        eng.run_device(*dev)
        s = eng.finish()
        # (lengths that leave every window count alone refute the pass only where it kept the geometry it held: with
        # RAFT_NO_KEEP_GEOMETRY=1 the scan runs over the new lengths and the pass stands)
        assert what == "same_windows" or not (s.flags & SPECULATED)
        assert bool(s.flags & engine.SUM_RERUN) != bool(s.flags & SPECULATED), (what, s.flags)   # refuted: run again, nothing remembered
        assert_same_result(_result(eng, s), want, what)
        # ... and the context is itself again afterwards
        eng.run_device(*dev); s = eng.finish()
        assert_same_result(_result(eng, s), want, what + ", next pass")
    eng.close()


def test_detecting_context_speculates_too_and_keeps_detecting():
    """symmetric_mode = -1: the mirror of record 0 is searched in every pass, speculative or not (chop.hpp:171-184)."""
    import torch
    from raft_amd import engine
    rng = np.random.default_rng(3)
    n_reads, n = 1500, 20000
    rl = rng.integers(3000, 40000, n_reads).astype(np.int32)
    qid = np.sort(rng.integers(0, n_reads, n)).astype(np.int32)
    tid = rng.integers(0, n_reads, n).astype(np.int32)
    a = (rng.random(n) * rl[qid] * 0.8).astype(np.int32); b = np.minimum(rl[qid], a + 1 + (rng.random(n) * rl[qid] * 0.2).astype(np.int32)).astype(np.int32)
    ta = (rng.random(n) * rl[tid] * 0.8).astype(np.int32); tb = np.minimum(rl[tid], ta + 1 + (rng.random(n) * rl[tid] * 0.2).astype(np.int32)).astype(np.int32)
    order = np.argsort(tid, kind="stable")
    sym = tuple(np.concatenate([x, y[order]]) for x, y in ((qid, tid), (a, ta), (b, tb), (tid, qid), (ta, a), (tb, b)))
    p = RaftParams(est_cov=10)
    want = oracle_run(p, rl, *sym)
    assert want["symmetric"] == 1
    dev = [torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0") for x in (rl,) + sym]
    eng = engine.Engine(p, device=0)
    for it in range(3):
        eng.run_device(*dev); s = eng.finish()
        assert bool(s.flags & SPECULATED) == (it > 0)
        assert_same_result(_result(eng, s), want, f"pass {it}")
    # the mirror goes away (record 0's mirror gets another target start): same shape, not symmetric any more -- the target sides of the
    # second half (= the query sides of the first) are then piled up a second time, as the reference does (chop.hpp:165-169)
    mirror = int(np.flatnonzero((sym[0][n:] == sym[3][0]) & (sym[3][n:] == sym[0][0]) & (sym[4][n:] == sym[1][0]) & (sym[5][n:] == sym[2][0]))[0]) + n
    dev[5][mirror] = max(0, int(sym[4][mirror]) - 1) if int(sym[4][mirror]) > 0 else int(sym[4][mirror]) + 1
    cols = [t.cpu().numpy() for t in dev]
    want2 = oracle_run(p, *cols)
    assert want2["symmetric"] == 0
    eng.run_device(*dev); s = eng.finish()
    assert_same_result(_result(eng, s), want2, "mirror gone")
    eng.close()


def test_a_deep_pile_appears_in_a_stream_that_had_none():
    """A speculative pass over a stream whose last pass listed no deep tile does not launch the 32-bit side kernel.  Same counts, same
    run, same window count -- but now 40,000 records sit on one read: the wave kernel finds no room for the tile, the pass is run
    again the long way (RERUN), and the result is the oracle's; the passes after that launch the side kernel and need no re-run."""
    import torch
    from raft_amd import engine
    p = RaftParams(est_cov=8, symmetric_mode=1)
    rng = np.random.default_rng(21)
    n_reads, n = 1200, 48000
    rl = rng.integers(30000, 60000, n_reads).astype(np.int32)
    qid = np.repeat(np.arange(n_reads, dtype=np.int32), n // n_reads)               # 40 records per read, one sorted run
    a = (rng.random(n) * rl[qid] * 0.5).astype(np.int32); b = (a + 1 + (rng.random(n) * rl[qid] * 0.4).astype(np.int32)).astype(np.int32)
    dev = [torch.from_numpy(x).to("cuda:0") for x in (rl, qid, a, b)]
    eng = engine.Engine(p, device=0)
    for _ in range(3):
        eng.run_device(*dev); s = eng.finish()
    assert s.flags & SPECULATED and not (s.flags & 4)
    qid2 = np.sort(np.concatenate([qid[::6][:n - 40000], np.full(40000, 700, np.int32)])).astype(np.int32)      # 8,000 records spread over the reads + the pile
    a2 = (rng.random(n) * rl[qid2] * 0.5).astype(np.int32); b2 = (a2 + 1 + (rng.random(n) * rl[qid2] * 0.4).astype(np.int32)).astype(np.int32)
    want = oracle_run(p, rl, qid2, a2, b2, qid2, a2, b2); want["symmetric"] = 1
    assert want["cov"].max() >= 10000
    for t, x in zip(dev[1:], (qid2, a2, b2)):
        t.copy_(torch.from_numpy(x))
    flags = []
    for it in range(3):
        eng.run_device(*dev); s = eng.finish()
        flags.append(s.flags)
        assert_same_result(_result(eng, s), want, f"deep pile, pass {it}")
    assert flags[0] & 8 and flags[0] & 4 and not (flags[0] & SPECULATED), flags         # re-run, deep tiles taken
    assert all(f & 4 and not (f & 8) for f in flags[1:]), flags
    eng.close()


def test_another_set_of_reads_in_between_does_not_leave_its_geometry_behind():
    """A speculative pass keeps the per-read geometry the context holds when nobody has written it since the pass it is built on.  A
    grouped pass over OTHER reads writes it: the next pass over the first set -- same buffers, same shape, speculative -- must not run
    on the other set's window offsets."""
    import torch
    from raft_amd import engine, hostio
    p = RaftParams(est_cov=8, symmetric_mode=1)
    rl, (qid, a, b) = _set(11)
    want = oracle_run(p, rl, qid, a, b, qid, a, b); want["symmetric"] = 1
    dev = [torch.from_numpy(x).to("cuda:0") for x in (rl, qid, a, b)]
    rl_o, (qid_o, a_o, b_o) = _set(12, n_reads=3000, n=40000, two_runs=False)      # as many reads, other lengths
    want_o = oracle_run(p, rl_o, qid_o, a_o, b_o, qid_o, a_o, b_o); want_o["symmetric"] = 1
    off_o = hostio.group_offsets(rl_o.size, qid_o)
    eng = engine.Engine(p, device=0)
    for it in range(3):
        eng.run_device(*dev); s = eng.finish()
    assert s.flags & SPECULATED
    assert_same_result(_result(eng, s), want, "first set")
    eng.run_host_grouped(rl_o, off_o, a_o, b_o); s = eng.finish()
    assert_same_result(_result(eng, s), want_o, "the other set, grouped")
    for it in range(2):
        eng.run_device(*dev); s = eng.finish()
        assert_same_result(_result(eng, s), want, f"first set again, pass {it}")
    assert s.flags & SPECULATED
    eng.close()


# ---- directed: what the shape key does not cover ---------------------------------------------------------------------------------
# Each test warms a context into speculation over fixed buffers (SPECULATED and KEPT_GEOMETRY), makes ONE change the key does not
# look at, and checks the next passes against the oracle and their flags against what the engine promises.

def _warm(eng, dev, want, what="warm-up"):
    from raft_amd import engine
    for it in range(3):
        eng.run_device(*dev); s = eng.finish()
        assert_same_result(_result(eng, s), want, f"{what}, pass {it}")
    assert s.flags & engine.SUM_SPECULATED and s.flags & engine.SUM_KEPT_GEOMETRY, s.flags
    return s


def _passes(eng, dev, want, what, n=2, fetch=None):
    flags = []
    for it in range(n):
        eng.run_device(*dev); s = eng.finish()
        flags.append(s.flags)
        assert_same_result((fetch or _result)(eng, s), want, f"{what}, pass {it}")
    return flags


def _runs_setup(seed=31, **kw):
    import torch
    p = RaftParams(**dict(dict(est_cov=8, symmetric_mode=1), **kw))
    rl, (qid, a, b) = _set(seed)
    dev = [torch.from_numpy(x).to("cuda:0") for x in (rl, qid, a, b)]
    return p, (rl, qid, a, b), dev


def _want1(p, rl, qid, a, b):
    w = oracle_run(p, rl, qid, a, b, qid, a, b); w["symmetric"] = 1
    return w


def test_force_bucket_toggled_between_speculative_passes():
    from raft_amd import engine
    p, cols, dev = _runs_setup()
    want = _want1(p, *cols)
    eng = engine.Engine(p, device=0)
    _warm(eng, dev, want)
    eng.set_tuning(0, True)
    f = _passes(eng, dev, want, "force_bucket on")
    assert not any(x & engine.SUM_SPECULATED for x in f), f          # (the general bucketing never speculates)
    eng.set_tuning(0, False)
    f = _passes(eng, dev, want, "force_bucket off")
    assert not f[0] & engine.SUM_SPECULATED and f[1] & engine.SUM_SPECULATED and f[1] & engine.SUM_KEPT_GEOMETRY, f
    eng.close()


def test_output_width_changes_between_speculative_passes():
    from raft_amd import engine, hostio
    p, cols, dev = _runs_setup()
    want = _want1(p, *cols)
    eng = engine.Engine(p, device=0)
    _warm(eng, dev, want)

    def packed(eng, s, w):
        got = _result(eng, s)                                   # (int32 decoded on the device) ...
        if w in (1, 2):                                          # ... and the encoding the pass wrote, as it travels
            pk = eng.fetch_packed(width=w)
            assert np.array_equal(hostio.unpack_coverage(pk["cov8"], pk["exc_index"], pk["exc_value"]), want["cov"]), w
        elif w == 8:
            d4 = eng.fetch_delta4()
            assert np.array_equal(hostio.unpack_coverage_d4(s.n_bins, d4["cov_nib"], d4["cov_anchor"], d4["exc_index"], d4["exc_value"]),
                                  want["cov"])
        return got
    for w in (1, 2, 8, 4):
        eng.set_output_width(w)
        f = _passes(eng, dev, want, f"width {w}", fetch=lambda e, s, w=w: packed(e, s, w))
        assert all(x & engine.SUM_SPECULATED and x & engine.SUM_KEPT_GEOMETRY for x in f), (w, f)
    eng.close()


def test_emit_cuts_toggled_between_speculative_passes():
    from raft_amd import engine
    p, cols, dev = _runs_setup()
    want = _want1(p, *cols)
    eng = engine.Engine(p, device=0)
    _warm(eng, dev, want)
    for on in (False, True):
        eng.set_emit_cuts(on)
        f = _passes(eng, dev, want, f"emit_cuts {on}")
        assert all(x & engine.SUM_SPECULATED and x & engine.SUM_KEPT_GEOMETRY for x in f), (on, f)
    eng.close()


@pytest.mark.parametrize("change", [dict(est_cov=11), dict(cov_mul=2.0), dict(flanking_length=400), dict(read_length=15000),
                                    dict(overlap_length=2000), dict(repeat_length=9960)],
                         ids=["est_cov", "cov_mul", "flank", "read_length", "overlap_length", "repeat_length_same_minbins"])
def test_params_that_keep_minbins_between_speculative_passes(change):
    """Parameters outside the shape key change the results but not the per-read geometry: the passes stay speculative, keep the
    geometry, and equal the oracle under the NEW parameters."""
    from raft_amd import engine
    p, cols, dev = _runs_setup()
    eng = engine.Engine(p, device=0)
    _warm(eng, dev, _want1(p, *cols))
    p2 = RaftParams(**dict(p.__dict__, **change))
    assert (p2.repeat_length + p2.reso - 1) // p2.reso == (p.repeat_length + p.reso - 1) // p.reso
    want2 = _want1(p2, *cols)
    eng.set_params(p2)
    f = _passes(eng, dev, want2, f"set_params {change}")
    assert all(x & engine.SUM_SPECULATED and x & engine.SUM_KEPT_GEOMETRY for x in f), f
    eng.close()


def test_params_that_change_minbins_are_not_speculated():
    from raft_amd import engine
    p, cols, dev = _runs_setup()
    eng = engine.Engine(p, device=0)
    _warm(eng, dev, _want1(p, *cols))
    p2 = RaftParams(**dict(p.__dict__, repeat_length=8000))
    want2 = _want1(p2, *cols)
    eng.set_params(p2)
    f = _passes(eng, dev, want2, "repeat_length 8000", n=3)
    assert not f[0] & engine.SUM_SPECULATED, f
    assert all(x & engine.SUM_SPECULATED and x & engine.SUM_KEPT_GEOMETRY for x in f[1:]), f
    eng.close()


def _detect_cols(seed=41):
    rng = np.random.default_rng(seed)
    n_reads, n = 1500, 20000
    rl = rng.integers(3000, 40000, n_reads).astype(np.int32)
    qid = np.sort(rng.integers(0, n_reads, n)).astype(np.int32)
    tid = rng.integers(0, n_reads, n).astype(np.int32)
    a = (rng.random(n) * rl[qid] * 0.8).astype(np.int32); b = np.minimum(rl[qid], a + 1 + (rng.random(n) * rl[qid] * 0.2).astype(np.int32)).astype(np.int32)
    ta = (rng.random(n) * rl[tid] * 0.8).astype(np.int32); tb = np.minimum(rl[tid], ta + 1 + (rng.random(n) * rl[tid] * 0.2).astype(np.int32)).astype(np.int32)
    order = np.argsort(tid, kind="stable")
    return [rl] + [np.ascontiguousarray(np.concatenate([x, y[order]]), dtype=np.int32)
                   for x, y in ((qid, tid), (a, ta), (b, tb), (tid, qid), (ta, a), (tb, b))]


@pytest.mark.parametrize("mode", [0, -1])
def test_target_columns_replaced_behind_the_same_query_column(mode):
    """New tid / ts / te tensors, same qid: symmetric_mode = 0 never speculates; a detecting context speculates on copies of the same
    targets, and targets without the mirror of record 0 send the pass the long way (and the context off its symmetric guess)."""
    import torch
    from raft_amd import engine
    S, K = engine.SUM_SPECULATED, engine.SUM_KEPT_GEOMETRY
    cols = _detect_cols()
    p = RaftParams(est_cov=10, symmetric_mode=mode)
    n = cols[1].size // 2
    broken = [c.copy() for c in cols]
    m = int(np.flatnonzero((cols[1][n:] == cols[4][0]) & (cols[4][n:] == cols[1][0]) & (cols[5][n:] == cols[2][0]) & (cols[6][n:] == cols[3][0]))[0]) + n
    broken[5][m] += 1 if broken[5][m] == 0 else -1
    other = [c.copy() for c in broken]                                                 # more target starts moved, still no mirror
    k = np.random.default_rng(9).choice(cols[1].size, 500, replace=False)
    other[5][k] = 0
    want_b, want_o = oracle_run(p, *broken), oracle_run(p, *other)
    assert want_b["symmetric"] == 0 and want_o["symmetric"] == 0
    dev = [torch.from_numpy(x).to("cuda:0") for x in (cols if mode == -1 else broken)]
    eng = engine.Engine(p, device=0)
    if mode == -1:
        want = oracle_run(p, *cols)
        assert want["symmetric"] == 1
        _warm(eng, dev, want)
        dev2 = dev[:4] + [torch.from_numpy(x).to("cuda:0") for x in cols[4:]]          # new tensors, same targets
        f = _passes(eng, dev2, want, "same targets, new tensors")
        assert all(x & S and x & K for x in f), f
        dev3 = dev[:4] + [torch.from_numpy(x).to("cuda:0") for x in broken[4:]]        # new tensors, the mirror gone
        f = _passes(eng, dev3, want_b, "mirror gone")
        assert not f[0] & S and f[0] & engine.SUM_RERUN and not f[1] & S, f
        f = _passes(eng, dev2, want, "mirror back", n=3)                                # detected again, then speculated again
        assert not f[0] & S and f[2] & S, f
    else:
        for it, (tcols, w) in enumerate(((broken[4:], want_b), (other[4:], want_o), (broken[4:], want_b))):
            d = dev[:4] + [torch.from_numpy(x).to("cuda:0") for x in tcols]
            f = _passes(eng, d, w, f"mode 0, target set {it}")
            assert not any(x & S for x in f), f
    eng.close()


def test_pipelined_and_host_windows_passes_in_between():
    """Other entry points on the same context between speculative passes: the host pipeline (its lanes, or the context itself for a
    one-piece job) and a grouped pass over window records, which writes the geometry -- the next plain pass may speculate, but must
    not keep what the grouped pass left."""
    from raft_amd import engine, hostio
    S, K = engine.SUM_SPECULATED, engine.SUM_KEPT_GEOMETRY
    p, cols, dev = _runs_setup()
    want = _want1(p, *cols)
    rl_o, (qid_o, a_o, b_o) = _set(32, n_reads=3000, n=60000)                          # the same counts, other reads
    want_o = _want1(p, rl_o, qid_o, a_o, b_o)
    eng = engine.Engine(p, device=0)
    _warm(eng, dev, want)
    for n_chunks in (1, 3):
        res, s = eng.run_pipelined(rl_o, qid_o, a_o, b_o, n_chunks=n_chunks)
        assert np.array_equal(hostio.unpack_coverage(res["cov8"], res["exc_index"], res["exc_value"]), want_o["cov"])
        for k in ("cov_offset", "rep_offset", "rep_s", "rep_e", "frag_offset", "frag_begin", "frag_end"):
            assert np.array_equal(res[k], want_o[k]), (n_chunks, k)
        f = _passes(eng, dev, want, f"after run_pipelined, {n_chunks} chunks")
        assert f[1] & S and f[1] & K, f
    off = hostio.group_offsets(rl_o.size, qid_o)
    win = hostio.pack_windows(a_o, b_o, p.reso)
    eng.run_host_windows(rl_o, off, win); s = eng.finish()
    assert_same_result(_result(eng, s), want_o, "run_host_windows")
    f = _passes(eng, dev, want, "after run_host_windows")
    assert f[0] & S and not f[0] & K and f[1] & S and f[1] & K, f
    eng.close()


def test_outputs_device_hands_out_the_geometry_and_the_next_pass_scans_it_again():
    """raft_hip_outputs_device returns the context's own offsets, and cov_offset is the geometry a speculative pass may keep.  The pass
    after the call scans it again (no KEPT_GEOMETRY), the one after that keeps it again; a caller's in-bounds write into the offsets
    -- monotone, ends unchanged, one interior offset moved by one window -- does not reach the next pass's results."""
    import torch
    from raft_amd import engine
    S, K = engine.SUM_SPECULATED, engine.SUM_KEPT_GEOMETRY
    p, cols, dev = _runs_setup()
    want = _want1(p, *cols)
    eng = engine.Engine(p, device=0)
    _warm(eng, dev, want)
    o = eng.outputs_device()
    assert np.array_equal(o["cov_offset"].cpu().numpy(), want["cov_offset"])
    f = _passes(eng, dev, want, "after outputs_device")
    assert f[0] & S and not f[0] & K and f[1] & S and f[1] & K, f
    o = eng.outputs_device()
    co = o["cov_offset"]
    h = co.cpu().numpy()
    j = int(np.flatnonzero(h[2:-1] - h[1:-2] >= 2)[0]) + 1
    co[j] += 1                                                                          # read j - 1 one window longer, read j one shorter
    torch.cuda.synchronize()
    e = co.cpu().numpy()
    assert (np.diff(e) >= 0).all() and e[0] == h[0] and e[-1] == h[-1] and (e != h).sum() == 1
    f = _passes(eng, dev, want, "after a write into cov_offset")
    assert f[0] & S and not f[0] & K, f
    eng.close()


def test_run_device_after_tensors_were_resized_in_place():
    """resize_ to fewer elements keeps a tensor's address and storage.  The next run_device must see the tensors as they are now:
    the oracle's result over them, or a ValueError / TypeError -- never the result for the old lengths.  Three cases, each after
    speculative passes: read_len shorter (stale n_reads), all six PAF columns shorter alike (stale n_rec), one column shorter."""
    import torch
    from raft_amd import engine
    p, (rl, qid, a, b), _ = _runs_setup()
    keep = qid < 2500                                                                   # reads 2500.. have no records
    qid, a, b = qid[keep], a[keep], b[keep]
    # (symmetric_mode = 1: the target columns are not read, but handed over -- all seven tensors take part in the call)
    dev = [torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0") for x in (rl, qid, a, b, qid, a, b)]
    eng = engine.Engine(p, device=0)
    _warm(eng, dev, _want1(p, rl, qid, a, b))

    def run_or_reject(want, what):
        try:
            eng.run_device(*dev)
        except (ValueError, TypeError):
            return
        s = eng.finish()
        assert_same_result(_result(eng, s), want, what)

    ptr = dev[0].data_ptr()
    dev[0].resize_(2500)
    assert dev[0].data_ptr() == ptr
    want = _want1(p, rl[:2500], qid, a, b)
    run_or_reject(want, "read_len resized to 2500")
    f = _passes(eng, dev, want, "read_len 2500, again")
    assert f[1] & engine.SUM_SPECULATED, f
    m = qid.size - 1000                                                                 # a prefix of the two sorted runs
    ptrs = [t.data_ptr() for t in dev[1:]]
    for t in dev[1:]:
        t.resize_(m)
    assert [t.data_ptr() for t in dev[1:]] == ptrs
    run_or_reject(_want1(p, rl[:2500], qid[:m], a[:m], b[:m]), f"PAF columns resized to {m}")
    # one coordinate column shorter than the others: not a valid input any more
    dev[2].resize_(m - 10)
    with pytest.raises((ValueError, TypeError)):
        eng.run_device(*dev)
        eng.finish()
    eng.close()


def test_a_negative_length_after_outputs_device_is_rejected_every_time():
    """A read of length 0, then outputs_device (the next pass scans the geometry again), then a negative length in the same buffer:
    the speculative pass that scans reports ERR_PARAM at that read -- and so does the pass after it, which must not keep a geometry
    (and a copy of the lengths) that scan made while it met the error."""
    import torch
    from raft_amd import engine
    p, (rl, qid, a, b), _ = _runs_setup()
    r = 1234
    rl = rl.copy(); rl[r] = 0
    keep = qid != r
    qid, a, b = qid[keep], a[keep], b[keep]
    dev = [torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0") for x in (rl, qid, a, b)]
    eng = engine.Engine(p, device=0)
    _warm(eng, dev, _want1(p, rl, qid, a, b))
    eng.outputs_device()
    dev[0][r] = -5
    torch.cuda.synchronize()
    for it in range(2):
        eng.run_device(*dev)
        with pytest.raises(engine.RaftError) as e:
            eng.finish()
        assert e.value.code == engine.ERR_PARAM and e.value.index == r, (it, e.value.code, e.value.index)
    # the length put right again: the oracle's result
    dev[0][r] = 0
    _passes(eng, dev, _want1(p, rl, qid, a, b), "length 0 again")
    eng.close()
