"""GPU: the chunked host pipeline (raft_hip_run_pipelined / raft_hip_run_multi / _grouped / _windows and the host-routed path of
raft_amd/csrc/engine_pipeline.hip) on its structural edges: the cases of tests/pipeline_cases.py -- chunks without records or windows,
chunks of one record, more chunks than reads, lanes or ring slots, runs absent from chunks, jobs whose repeats fill their room, gaps that
close_gaps closes or leaves, exceptions that take the shared cursor in any order, delta4 chunks inside, on and across the anchors' blocks --
through every form of the entry that applies, on 1, 2 and 3 contexts, bit-exact against the oracle on the whole set; that the route the
case claims is the route that ran; the capacities at and one below what the placement needs; data errors in the first, a middle and the
last chunk; and that the other contexts have their own parameters again afterwards.  tests/test_pipeline_cases.py holds the cases' claims
against the real planner on the CPU."""
import re

import numpy as np
import pytest
from pipeline_cases import CASES, CONTEXTS, D4_BLOCK, ROUTED, by_name, model_routed
from raft_testlib import RaftParams, oracle_run
from test_gpu_delta4 import check_pipelined_d4
from test_gpu_grouped import check_pipelined

pytestmark = pytest.mark.gpu

FORMS = ("derived", "columns", "grouped", "windows")
LIMIT = {1: 255, 2: 65535}
OTHER = RaftParams(est_cov=3, reso=7, symmetric_mode=1)     # what the contexts other than the first are made with: never the job's
STAMP = re.compile(r"PIPE chunk\s+(\d+) pass done")
LAST = {"stamps": set()}                                    # chunk indices the last call of run_form stamped, also when it raised


@pytest.fixture(scope="module")
def engs():
    """One set of contexts for the whole module: lanes' buffers, derive rings and staging blocks are reused from case to case."""
    from raft_amd import engine
    es = [engine.Engine(CASES[0].p, device=0)] + [engine.Engine(OTHER, device=0) for _ in range(max(CONTEXTS) - 1)]
    for e, p in zip(es, [CASES[0].p, OTHER, OTHER]):
        own_pass_equals_oracle(e, p, "two_by_two/c2", "a context's first pass")      # (every context holds a pass of its own to lose)
    yield es
    for e in es:
        e.close()


def large_small(cases):
    """Largest, smallest, second largest, second smallest ...: buffers shrink and grow in both directions."""
    by_size = sorted(cases, key=lambda c: (-c.n_rec, c.name))
    out = []
    while by_size:
        out.append(by_size.pop(0))
        if by_size:
            out.append(by_size.pop())
    return out


def run_form(es, case, form, width, monkeypatch, capfd, out=None, cols=None):
    """One call of the entry; (results, summary, chunk indices with a "pass done" stamp)."""
    from raft_amd import hostio
    eng, others = es[0], es[1:]
    q, s, e = cols or case.cols
    if out is None:
        out = eng.host_output_buffers(case.read_len, pinned=False, width=width)
    if width == 8:
        out["cov_nib"][:] = 0xA5; out["cov_anchor"][:] = -7          # (stale bytes of the pass before must not survive)
    monkeypatch.setenv("RAFT_PIPE_TRACE", "1")
    if form == "columns":
        monkeypatch.setenv("RAFT_NO_DERIVE", "1")
    else:
        monkeypatch.delenv("RAFT_NO_DERIVE", raising=False)
    capfd.readouterr()
    try:
        if form in ("derived", "columns"):
            res, summ = eng.run_pipelined(case.read_len, q, s, e, n_chunks=case.n_chunks, out=out, others=others)
        elif form == "grouped":
            res, summ = eng.run_pipelined_grouped(case.read_len, case.offsets, s, e, n_chunks=case.n_chunks, out=out, others=others)
        else:
            win = hostio.pack_windows(s, e, case.p.reso)
            res, summ = eng.run_pipelined_windows(case.read_len, case.offsets, win, n_chunks=case.n_chunks, out=out, others=others)
    finally:
        LAST["stamps"] = {int(k) for k in STAMP.findall(capfd.readouterr().err)}
    return res, summ, LAST["stamps"]


def holds_no_pass(eng):
    from raft_amd import engine
    with pytest.raises(engine.RaftError) as e:
        eng.fetch()
    return e.value.code == engine.ERR_STATE


def check_result(case, width, res, s, what):
    from raft_amd import hostio
    want = case.oracle()
    if width == 8:
        check_pipelined_d4(res, s, want, what)
        n = want["cov"].size
        for b in range(1, (n + D4_BLOCK - 1) // D4_BLOCK):           # every block stands on its own anchor
            lo = b * D4_BLOCK
            keep = res["exc_index"] >= lo
            got = hostio.unpack_coverage_d4(n - lo, res["cov_nib"][lo // 2:], res["cov_anchor"][b:], res["exc_index"][keep] - lo, res["exc_value"][keep])
            assert np.array_equal(got, want["cov"][lo:]), (what, "decoded from block", b)
    else:
        check_pipelined(res, s, want, what)
        deep = np.flatnonzero(want["cov"] >= LIMIT[width])
        assert np.array_equal(res["exc_index"], deep) and np.array_equal(res["exc_value"], want["cov"][deep]), what   # (ascending over the whole job)
    for k in ("rep_offset", "frag_offset", "cov_offset"):
        assert res[k].size == case.n_reads + 1 and res[k][-1] == want[k][-1], (what, k)


def check_route(es, case, form, width, s, stamps, what):
    """The route the case claims is the one that ran."""
    n_ctx, plan = len(es), case.plan_for(width)
    grouped = form in ("grouped", "windows")
    if plan is not None:
        assert stamps == set(range(len(plan))), (what, sorted(stamps))
        used = min(n_ctx, len(plan))
        assert s.n_devices_used == used and s.n_segments == case.n_runs, (what, s.n_devices_used, s.n_segments)
        assert all(holds_no_pass(e) for e in es[:used]), what
    elif case.route == "routed" and width != 8:
        q = case.cols[0]
        recs6 = [(int(x), 0, 0, int(x), 0, 0) for x in q]
        n_ch = len(model_routed(case.n_reads, recs6, 1, case.n_chunks, n_ctx)) - 1
        assert not stamps and s.n_devices_used == min(n_ctx, n_ch) and s.n_segments == 1, (what, sorted(stamps), s.n_devices_used, s.n_segments)
        assert all(holds_no_pass(e) for e in es[:s.n_devices_used]), what
    else:
        # one piece: on the first context, which holds the pass; only a plan that its chunks refuted ("redo") has left stamps
        assert case.route == "redo" or not stamps, (what, sorted(stamps))
        assert s.n_devices_used == 1 and s.n_segments == (case.n_runs if grouped else case.descents), (what, s.n_devices_used, s.n_segments)
        got, want = es[0].fetch(), case.oracle()
        for k in ("cov_offset", "rep_offset", "rep_s", "rep_e", "frag_offset", "frag_begin", "frag_end"):
            assert np.array_equal(got[k], want[k]), (what, "the first context's own pass", k)


def run_and_check(es, case, form, width, monkeypatch, capfd, what=""):
    what = f"{case.name} {form} width {width} contexts {len(es)} {what}"
    res, s, stamps = run_form(es, case, form, width, monkeypatch, capfd)
    check_result(case, width, res, s, what)
    check_route(es, case, form, width, s, stamps, what)


@pytest.mark.parametrize("n_ctx", CONTEXTS)
@pytest.mark.parametrize("form", FORMS)
def test_every_case_equals_the_oracle_by_its_claimed_route(engs, form, n_ctx, monkeypatch, capfd):
    cases = large_small([c for c in CASES if form in c.forms])
    assert len(cases) >= 20
    for case in cases:
        for width in case.widths:
            for rep in range(2):
                run_and_check(engs[:n_ctx], case, form, width, monkeypatch, capfd, f"pass {rep}")


def own_pass_equals_oracle(eng, p, case, what):
    """A pass of the context's own, under ITS parameters."""
    q, s, e = by_name(case).cols
    rl = by_name(case).read_len
    want = oracle_run(p, rl, q, s, e, q, s, e)
    eng.run_host(rl, q, s, e, None, None, None)
    summ = eng.finish()
    got = eng.fetch()
    for k in ("cov_offset", "cov", "rep_offset", "rep_s", "rep_e", "frag_offset", "frag_begin", "frag_end"):
        assert np.array_equal(got[k], want[k]), (what, k)
    assert summ.high_cov == want["high_cov"] and summ.total_windows == want["total_windows"], what


@pytest.mark.parametrize("n_ctx", [2, 3])
def test_the_other_contexts_have_their_own_parameters_again(engs, n_ctx, monkeypatch, capfd):
    """raft_hip.h: ctxs[0]'s parameters apply to all for the duration of the call.  After a chunked job, a job the chunks refuted, a
    refused one and a routed one every other context computes under the parameters it was made with."""
    es = engs[:n_ctx]
    from raft_amd import engine
    for name in ("nine/c9", "descent/c4"):
        run_and_check(es, by_name(name), "derived", 1, monkeypatch, capfd)
        for d, e in enumerate(es[1:], 1):
            own_pass_equals_oracle(e, OTHER, "eight/c8", f"context {d} after {name}")
    case = by_name("reps_every/c4")
    out = es[0].host_output_buffers(case.read_len, pinned=False)
    small = dict(out, rep_s=out["rep_s"][:1], rep_e=out["rep_e"][:1])
    with pytest.raises(engine.RaftError) as err:
        run_form(es, case, "grouped", 1, monkeypatch, capfd, out=small)
    assert err.value.code == engine.ERR_TOO_LARGE and not LAST["stamps"]
    for d, e in enumerate(es[1:], 1):
        own_pass_equals_oracle(e, OTHER, "eight/c8", f"context {d} after a refused job")
    for rc in ROUTED:
        es[0].set_params(rc.p)
        res, s = es[0].run_pipelined(rc.read_len, *rc.cols, n_chunks=rc.n_chunks, others=es[1:])
        check_pipelined(res, s, rc.oracle(), f"{rc.name} contexts {n_ctx}")
        for d, e in enumerate(es[1:], 1):
            own_pass_equals_oracle(e, OTHER, "eight/c8", f"context {d} after {rc.name}")
        # ... and the first one its own, flag included
        es[0].run_host(rc.read_len, *rc.cols)
        assert es[0].finish().symmetric == rc.oracle()["symmetric"]
    es[0].set_params(CASES[0].p)


@pytest.mark.parametrize("n_ctx", CONTEXTS)
@pytest.mark.parametrize("case", ROUTED, ids=lambda c: c.name)
def test_routed_edges(engs, case, n_ctx, monkeypatch, capfd):
    """The host-routed path (ids in no order, the flag not asserted) where its bounds leave chunks of one read, chunks without intervals,
    fewer chunks than contexts."""
    es = engs[:n_ctx]
    want = case.oracle()
    es[0].set_params(case.p)
    monkeypatch.setenv("RAFT_PIPE_TRACE", "1")
    try:
        for width in (1, 2):
            out = es[0].host_output_buffers(case.read_len, pinned=False, width=width)
            for rep in range(2):
                capfd.readouterr()
                res, s = es[0].run_pipelined(case.read_len, *case.cols, n_chunks=case.n_chunks, out=out, others=es[1:])
                what = f"{case.name} width {width} contexts {n_ctx} pass {rep}"
                assert not STAMP.findall(capfd.readouterr().err), what
                check_pipelined(res, s, want, what)
                deep = np.flatnonzero(want["cov"] >= LIMIT[width])
                assert np.array_equal(res["exc_index"], deep), what
                n_ch = len(case.bounds[n_ctx]) - 1
                assert s.n_devices_used == min(n_ctx, n_ch) and s.n_segments == 1 and s.symmetric == want["symmetric"], (what, s.n_devices_used)
                assert all(holds_no_pass(e) for e in es[:s.n_devices_used]), what
    finally:
        es[0].set_params(CASES[0].p)


def test_contexts_beyond_the_chunks_are_untouched(engs, monkeypatch, capfd):
    """Two chunks, three contexts: the third keeps the pass it holds."""
    third = engs[2]
    own_pass_equals_oracle(third, OTHER, "five/c5", "before")
    held = third.fetch()
    for form in FORMS:
        run_and_check(engs, by_name("two_by_two/c2"), form, 1, monkeypatch, capfd)
        got = third.fetch()
        assert all(np.array_equal(got[k], held[k]) for k in held), form


@pytest.mark.parametrize("n_ctx", [2, 3])
def test_capacities_exactly_at_the_placement_s_sum_and_one_below(engs, n_ctx, monkeypatch, capfd):
    """Several contexts: the caller's rep_cap / frag_cap / cov8_cap at the sum of the jobs' rooms serve the job; one below is refused before
    anything runs; the same call with room succeeds on the same contexts."""
    from raft_amd import engine
    es, case = engs[:n_ctx], by_name("reps_mixed/c4")
    bins, rep, frag = case.jobs[n_ctx][1]
    assert rep > len(case.oracle()["rep_s"]) and frag > len(case.oracle()["frag_begin"])      # (the bounds, not the job's own counts)
    base = es[0].host_output_buffers(case.read_len, pinned=False)

    def sized(bins, rep, frag):
        return dict(base, cov8=base["cov8"][:bins], rep_s=base["rep_s"][:rep], rep_e=base["rep_e"][:rep], frag_begin=base["frag_begin"][:frag],
                    frag_end=base["frag_end"][:frag])
    for form in FORMS:
        res, s, stamps = run_form(es, case, form, 1, monkeypatch, capfd, out=sized(bins, rep, frag))
        check_result(case, 1, res, s, f"{form}: exactly at the sum")
        assert len(stamps) == len(case.plan)
        for what, caps in (("rep_cap", (bins, rep - 1, frag)), ("frag_cap", (bins, rep, frag - 1)), ("cov8_cap", (bins - 1, rep, frag))):
            with pytest.raises(engine.RaftError) as err:
                run_form(es, case, form, 1, monkeypatch, capfd, out=sized(*caps))
            assert err.value.code == engine.ERR_TOO_LARGE and not LAST["stamps"], (form, what, LAST["stamps"])
            res, s, stamps = run_form(es, case, form, 1, monkeypatch, capfd, out=sized(bins, rep, frag))
            check_result(case, 1, res, s, f"{form}: after a refused {what}")


def test_capacities_of_one_context_are_the_job_s_own_counts(engs, monkeypatch, capfd):
    """One context: the caller's capacities are the only limits -- the job's repeats and fragments exactly fit, one below is refused when
    the chunk that overflows takes its place; the same call with room succeeds."""
    from raft_amd import engine
    es, case = engs[:1], by_name("reps_mixed/c4")
    want = case.oracle()
    bins, rep, frag = want["cov"].size, len(want["rep_s"]), len(want["frag_begin"])
    base = es[0].host_output_buffers(case.read_len, pinned=False)

    def sized(bins, rep, frag):
        return dict(base, cov8=base["cov8"][:bins], rep_s=base["rep_s"][:rep], rep_e=base["rep_e"][:rep], frag_begin=base["frag_begin"][:frag],
                    frag_end=base["frag_end"][:frag])
    for form in FORMS:
        for what, caps in (("rep_cap", (bins, rep - 1, frag)), ("frag_cap", (bins, rep, frag - 1)), ("cov8_cap", (bins - 1, rep, frag))):
            with pytest.raises(engine.RaftError) as err:
                run_form(es, case, form, 1, monkeypatch, capfd, out=sized(*caps))
            assert err.value.code == engine.ERR_TOO_LARGE, (form, what)
            res, s, stamps = run_form(es, case, form, 1, monkeypatch, capfd, out=sized(bins, rep, frag))
            check_result(case, 1, res, s, f"{form}: exactly the job's counts after a refused {what}")
            assert stamps == set(range(len(case.plan))) and holds_no_pass(es[0]), (form, what)


ERRORS = (("read id beyond the reads", 0, 99), ("negative read id", 0, -1), ("negative start", 1, -5), ("end beyond the read", 2, 700))


@pytest.mark.parametrize("n_ctx", [1, 3])
@pytest.mark.parametrize("form", ["derived", "columns", "grouped"])
def test_data_errors_end_as_the_one_piece_pass_ends(engs, form, n_ctx, monkeypatch, capfd):
    """A bad record in the first, a middle and the last chunk (with three contexts: a chunk of each): the call ends as run_host + finish
    ends, with the record's index in the caller's stream; the same contexts then run the good case."""
    from raft_amd import engine
    es, case = engs[:n_ctx], by_name("nine/c9")
    for what, col, value in ERRORS:
        if form == "grouped" and col == 0:
            continue                                   # (grouped input has no query column)
        for at in (1, 13, 26):                         # chunks 0, 4 and 8 of nine
            cols = [c.copy() for c in case.cols]
            cols[col][at] = value
            with pytest.raises(engine.RaftError) as e0:
                es[0].run_host(case.read_len, *cols, None, None, None)
                es[0].finish()
            with pytest.raises(engine.RaftError) as e1:
                run_form(es, case, form, 1, monkeypatch, capfd, cols=cols)
            want_code = engine.ERR_READ_ID if col == 0 else engine.ERR_COORD
            assert (e1.value.code, e1.value.index) == (e0.value.code, e0.value.index) == (want_code, at), (what, at, e1.value.code, e1.value.index)
            run_and_check(es, case, form, 1, monkeypatch, capfd, f"after: {what} at {at}")
