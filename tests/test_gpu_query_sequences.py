"""GPU: the seven queries about a finished pass inside the long call sequences of tests/test_gpu_context_sequences.py, on ONE context.

The op list of a seed (tests/query_sequence_model.py) is that file's, pass by pass, with 0 to 3 queries behind every op: coverage_histogram,
read_stats, low_coverage, census, repeat_overlaps, fragment_overlaps and repeat_stats, over the caller's live device tensors or host
columns, against the context's own pass or a table given with the call.  The queries share state with the passes and with each other --
finished / pending_err, pass_width against the width set for the next pass, cov_valid, the exception list, the counts and the rep_* /
frag_* arrays of the last pass, the staging set and the decoded coverage, buffers grown by a larger call, input tensors the speculation
has keyed -- and only an interleaving shows what a query reads of it.

At every query op the answer equals the numpy model's over the oracle's result for the LAST FINISHED pass, exactly, or the call is
refused with the code the context model predicts (ERR_STATE without a finished pass, ERR_PARAM over another number of reads or with
min_anchor < 1), the context's message (raft_hip_last_error) names this very call, and the context goes on working.  Behind a
host-to-host job the context holds no pass, or the job's where the library served it in one piece -- a job of one chunk for sure, and
its pass is then expected like any other; else a query is refused with ERR_STATE or answers for that pass, all queries behind one job
alike.  At every pass op the read-back equals the oracle as in the query-free file, so no query wrote the pass, left a stale
cov_valid or disturbed a kept geometry; at the end of a seed the summary flags of its passes equal those of the query-free run of
the same seed (no query hands out geometry or unarms the speculation), and the last eight results a caller would still hold are
compared once more (a result is a copy, not a view of a buffer the next query overwrites).  A failing step prints its seed and the op
list up to it (replay: ``-k "seed_<n>"``).  The last test counts, per query, the answers behind a pass that went the long way, a
speculated one, one with kept geometry, a re-run and one with deep tiles, and the refusals.

Wall time on one MI355X, both files in one pytest run, 16 seeds x 60 steps each (the sum of their tests' call times): this file 3.9 s
behind test_gpu_context_sequences.py's 3.4 s, whose oracle results and query-free flag lists it then shares (run alone it makes those
itself: about 1.5 s more); 5.2 s against 3.4 s under RAFT_NO_SPECULATE=1, 5.1 s against 3.2 s under RAFT_DEEP_MIN=40.  These
times include the numpy models on the host's CPU (test_query_sequence_model.py prints their cost for one seed)."""
import os

import numpy as np
import pytest
import query_sequence_model as m
import test_gpu_context_sequences as plain
from context_model import describe

pytestmark = pytest.mark.gpu

MIN_PER_PATH = 5
HELD = 8
PATHS = ("long_way", "speculated", "kept_geometry", "rerun", "deep_tiles")

_flags: dict = {}           # seed -> the summary flags of its passes, with the queries in between
_answers: dict = {}         # seed -> [(query, flags of the last finished pass or None on the lent engine)]
_refusals: dict = {}        # seed -> [(query, code)]


def _tables(q, done, device):
    """(repeats, fragments) as the call takes them: None for the context's own pass, else the arrays, on the device for a live form."""
    if q["table"] == "own":
        return None, None
    import torch
    rep, frag = m.tables_of(q, done)
    if device:
        rep, frag = ([torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in t] for t in (rep, frag))
    return tuple(rep), tuple(frag)


def _call(eng, q, tensors, done, variant_now):
    name = q["q"]
    if name == "coverage_histogram":
        return eng.coverage_histogram()
    if name == "read_stats":
        return eng.read_stats() if q["threshold"] is None else eng.read_stats(m.threshold_of(q, done, variant_now))
    if name == "low_coverage":
        return eng.low_coverage(q["low_cov"], m.PERMILLE)
    live = q["records"] == "live"
    cols = m.records_of(q, tensors if live else None)
    sym = q["symmetric"]
    if name == "census":
        return eng.census(*cols, symmetric=sym)
    rep, frag = _tables(q, done, live)
    if name == "repeat_overlaps":
        return eng.repeat_overlaps(*cols, min_anchor=q["min_anchor"], symmetric=sym, repeats=rep)
    if name == "fragment_overlaps":
        return eng.fragment_overlaps(*cols, symmetric=sym, fragments=frag, repeats=rep)
    threshold = None if q["threshold"] is None else m.threshold_of(q, done, variant_now)
    return eng.repeat_stats(*cols, symmetric=sym, repeats=rep, threshold=threshold)


def run_with_queries(seed):
    """One seed's list on one Engine (plain.run_sequence runs the passes and hands every query op over)."""
    from raft_amd import engine
    assert (engine.ERR_PARAM, engine.ERR_STATE) == (m.ERR_PARAM, m.ERR_STATE)
    ops = m.generate_with_queries(seed)
    plan = {}
    ctx = m.Context()
    for i, e in enumerate(ops):
        if e["op"] == "query":
            plan[i] = (m.outcome(ctx, e), dict(ctx.done or ctx.job or {}) or None, ctx.variant, ctx.job and ctx.job["n"], ctx.done is not None)
        ctx.apply(e)
    held, answers, refusals = [], [], []

    def attempt(eng, q, done, variant_now, tensors, what):
        """The call -> (None, its answer), or (the code it was refused with, None) with the context's own message checked: there, and
        of this very call (a call refused without a message, or under the message an earlier call left, fails here)."""
        try:
            return None, _call(eng, q, tensors, done, variant_now)
        except engine.RaftError as ex:
            text = eng._lib.raft_hip_last_error(eng._ctx).decode()
            assert text.startswith(m.MESSAGE_NAME[q["q"]] + ": ") and len(text) > len(m.MESSAGE_NAME[q["q"]]) + 2, \
                f"{what}: refused with {ex.code} and the context's message {text!r}, which is not this call's"
            assert text in str(ex), (what, text, str(ex))
            return ex.code, None
    job_left = {}               # per host-to-host job: does the first context hold its pass (served in one piece) or none?

    def query(eng, st, flags, i, q):
        (kind, code), done, variant_now, job, finished = plan[i]
        assert variant_now == st["variant"] and finished == st["finished"], "the context model and the runner disagree"
        what = f"seed {seed}, step {i} ({q['q']}, {q['records']} records, {q['table']} table)"
        if kind == "error":
            got, _ = attempt(eng, q, done, variant_now, st["tensors"], what)
            assert got == code, f"{what}: {'answered' if got is None else 'refused with %d' % got}, the model says refused with {code}"
            refusals.append((q["q"], code))
            return
        if kind == "either":                                     # behind a host-to-host job (query_sequence_model.outcome)
            other_reads = q["records"] != "pass" and m.n_reads_of(q["set"]) != m.n_reads_of(done["set"])
            rc, got = attempt(eng, q, done, variant_now, st["tensors"], what)
            if rc is not None:
                holds = rc == m.ERR_PARAM
                assert rc == m.ERR_STATE or (holds and other_reads), f"{what}: refused with {rc} behind a host-to-host job"
                refusals.append((q["q"], rc))
            else:
                holds = True
                assert not other_reads, f"{what}: answered over another number of reads than the job's"
                exp = m.expected(q, done, variant_now)
                m.same_answer(q, got, exp, f"{what}, the pass a job served in one piece left")
                answers.append((q["q"], None))
                held.append((what, q, got, exp))
            assert job_left.setdefault(job, holds) == holds, \
                f"{what}: the context {'holds' if holds else 'does not hold'} the job's pass, an earlier query saw the opposite"
            del held[:-HELD]
            return
        exp = m.expected(q, done, variant_now)
        got = _call(eng, q, st["tensors"], done, variant_now)
        m.same_answer(q, got, exp, what)
        answers.append((q["q"], flags[-1] if q.get("on") != "eng2" and finished else None))
        held.append((what, q, got, exp))
        del held[:-HELD]

    flags = plain.run_sequence(seed, ops=ops, query=query)
    try:
        for what, q, got, exp in held:
            m.same_answer(q, got, exp, f"{what}, looked at again after the sequence's last op")
    except AssertionError as ex:
        raise AssertionError(f"{ex}\nreplay: -k 'seed_{seed}'; ops:\n{describe(ops)}") from ex
    _flags[seed], _answers[seed], _refusals[seed] = flags, answers, refusals
    return flags


def _plain_flags(seed):
    if seed not in plain._flags:
        plain._flags[seed] = plain.run_sequence(seed)
    return plain._flags[seed]


@pytest.mark.parametrize("seed", m.SEEDS, ids=[f"seed_{s}" for s in m.SEEDS])
def test_query_sequence(seed):
    """(Both files read RAFT_NO_SPECULATE and RAFT_NO_KEEP_GEOMETRY through the library alone: the two runs see the same switches.)"""
    flags = run_with_queries(seed)
    want = _plain_flags(seed)
    assert len(flags) == len(want), (seed, len(flags), len(want))
    differ = [(j, hex(a), hex(b)) for j, (a, b) in enumerate(zip(flags, want)) if a != b]
    assert not differ, f"seed {seed}: (pass, flags with queries, flags without) {differ[:8]}: a query changed what a later pass reports"


def _paths(f, engine):
    S, K = engine.SUM_SPECULATED, engine.SUM_KEPT_GEOMETRY
    return [name for name, on in (("long_way", not f & S), ("speculated", f & S), ("kept_geometry", f & K), ("rerun", f & engine.SUM_RERUN),
                                  ("deep_tiles", f & engine.SUM_DEEP_TILES)) if on]


def test_every_query_answered_behind_every_path():
    """Over all seeds (missing seeds are run here: -k on one seed leaves this test whole)."""
    from raft_amd import engine
    for seed in m.SEEDS:
        if seed not in _flags:
            run_with_queries(seed)
    counts = {q: dict.fromkeys(PATHS, 0) for q in m.QUERIES}
    lent = dict.fromkeys(m.QUERIES, 0)
    for seed in m.SEEDS:
        for q, f in _answers[seed]:
            if f is None:
                lent[q] += 1
            else:
                for p in _paths(f, engine):
                    counts[q][p] += 1
    refused = {q: sorted({c for s in m.SEEDS for x, c in _refusals[s] if x == q}) for q in m.QUERIES}
    print(f"\nquery sequences, {len(m.SEEDS)} seeds: answers behind each path {counts}; answers without a finished pass {lent}; refusals {refused}")
    need = ["long_way", "deep_tiles"]
    if not os.environ.get("RAFT_NO_SPECULATE"):
        need += ["speculated", "rerun"]
        if not os.environ.get("RAFT_NO_KEEP_GEOMETRY"):
            need += ["kept_geometry"]
    missing = {(q, p): counts[q][p] for q in m.QUERIES for p in need if counts[q][p] < MIN_PER_PATH}
    assert not missing, f"answers behind a path fewer than {MIN_PER_PATH} times: {missing}"
    for q in m.QUERIES:
        want = [] if q == "census" else [m.ERR_STATE] if q in m.QUERIES[:3] else [m.ERR_PARAM, m.ERR_STATE]
        assert refused[q] == want, (q, refused[q], want)


def test_a_refused_query_leaves_its_own_message():
    """The narrowest form of what the sequences check at every refusal: a context without a pass refuses the six queries that need one
    (and repeat_overlaps with min_anchor = 0 whatever it holds), on the host, and raft_hip_last_error then names the refusing call --
    not nothing, and not the message the call before it left."""
    from context_model import params_of
    from raft_amd import engine
    rl = np.array([1000, 2000], np.int32)
    rec = [np.array([v], np.int32) for v in (0, 10, 500, 1, 20, 700)]
    given = (np.array([0, 1, 1], np.int64), np.array([100], np.int32), np.array([300], np.int32))
    eng = engine.Engine(params_of(0, 0), device=0)
    calls = (("coverage_histogram", engine.ERR_STATE, lambda: eng.coverage_histogram()),
             ("read_stats", engine.ERR_STATE, lambda: eng.read_stats(5)),
             ("low_coverage", engine.ERR_STATE, lambda: eng.low_coverage(0)),
             ("repeat_overlaps", engine.ERR_STATE, lambda: eng.repeat_overlaps(rl, *rec, min_anchor=300)),
             ("fragment_overlaps", engine.ERR_STATE, lambda: eng.fragment_overlaps(rl, *rec)),
             ("repeat_overlaps", engine.ERR_PARAM, lambda: eng.repeat_overlaps(rl, *rec, min_anchor=0, repeats=given)),
             ("repeat_stats", engine.ERR_STATE, lambda: eng.repeat_stats(rl, *rec, repeats=given, threshold=5)))
    try:
        for name, code, call in calls:
            with pytest.raises(engine.RaftError) as ex:
                call()
            text = eng._lib.raft_hip_last_error(eng._ctx).decode()
            assert ex.value.code == code and text.startswith(m.MESSAGE_NAME[name] + ": ") and text in str(ex.value), (name, ex.value.code, text)
        got = eng.repeat_overlaps(rl, *rec, min_anchor=300, repeats=given)          # ... and the context goes on working
        assert got["n_records"] == 1 and got["q_touch"] == 1
    finally:
        eng.close()
