"""CPU: the op lists, the context model and the expected answers of tests/test_gpu_query_sequences.py (tests/query_sequence_model.py).

The generator is deterministic per seed and leaves the pass ops of context_model.generate as they are; a census of the op lists over all
seeds (CLASSES) fails on an empty class; the input pool is such that a stale answer would show -- wherever the last finished pass
differs from the one before it in an array the query reads, the two expected answers differ --; and the fast sibling of
test_repeat_stats_cases.repeat_stats_model equals that model on the model's own cases, where each of its planted mistakes differs.

Model cost (test_model_cost_of_one_seed prints it, `-s` shows it): the expected answers of seed 0 from a cold cache, oracle runs
included, took 0.8 s on one core of the build machine.  On the GPU machine, whose cores are faster, the whole of
test_gpu_query_sequences.py -- 16 seeds, these models included -- took 3.9 s behind the query-free file's 3.4 s."""
import time

import numpy as np
import pytest
import query_sequence_model as m
import test_repeat_overlaps_cases as ovl_cases
import test_repeat_stats_cases as rst_cases
from context_model import N_STEPS, PARAM_VARIANTS, PASS_OPS, generate

OTHERS = {q: tuple(x for x in m.QUERIES if x != q) for q in m.QUERIES}
# where a query form must land, over all seeds: (class, the values every form needs)
CLASSES = (
    ("width", (1, 2, 4, 8)),                   # behind a finished pass run under each output width
    ("kind", PASS_OPS),                        # the last pass op before it: each kind
    ("after", None),                           # directly behind a query of each OTHER kind (OTHERS)
    ("route", ("fetch", "packed")),            # directly behind a pass read back through fetch / through a packed route
    ("setting", m.SETTINGS),                   # behind such a change with no pass in between
    ("pipelined", ((),)),                      # behind a host-to-host job: the context holds no pass
)


MIN_PER_CLASS = 5


def walk(ops):
    """(context before the op, op) for every op of a list."""
    ctx = m.Context()
    for e in ops:
        yield ctx, e
        ctx.apply(e)


def form_of(q):
    return q["q"], q["records"], "given" if q["table"] == "given_large" else q["table"]


def test_generator_is_deterministic_per_seed():
    seen = set()
    fresh = {s: m._generate(s, N_STEPS, seen) for s in m.SEEDS}
    for s in m.SEEDS:
        assert m.generate_with_queries(s) == fresh[s] == m.generate_with_queries(s, N_STEPS)
    assert m.generate_with_queries(100, 20) == m.generate_with_queries(100, 20)
    assert m.generate_with_queries(0) != m.generate_with_queries(1)


def test_the_pass_ops_are_those_of_the_query_free_test():
    for s in m.SEEDS:
        ops = m.generate_with_queries(s)
        assert m.pass_ops(ops) == generate(s, N_STEPS)
        for run in _query_runs(ops):                              # 0 to 3 behind every op; ten on the lent engine, first, behind pipelined2
            lent = [q for q in run if q.get("on") == "eng2"]
            assert len(run) - len(lent) <= 3 and run[:len(lent)] == lent, run
        assert all(len(lent) == (10 if e["op"] == "pipelined2" else 0) for e, lent in _lent_runs(ops))
    assert {q["q"] for s in m.SEEDS for q in m.generate_with_queries(s) if q["op"] == "query"} == set(m.QUERIES)


def _lent_runs(ops):
    """(op, the queries on the lent engine directly behind it)"""
    for i, e in enumerate(ops):
        if e["op"] != "query":
            n = 0
            while i + 1 + n < len(ops) and ops[i + 1 + n].get("on") == "eng2":
                n += 1
            yield e, ops[i + 1:i + 1 + n]


def _query_runs(ops):
    run = []
    for e in ops[1:]:
        if e["op"] == "query":
            run.append(e)
        else:
            yield run
            run = []
    yield run


def test_census_of_the_op_lists():
    seen = set()
    shrinks = grows = 0
    rank = {"given": 1, "given_large": 2}
    for s in m.SEEDS:
        prev = None
        for ctx, e in walk(m.generate_with_queries(s)):
            if e["op"] == "query" and e.get("on") != "eng2":
                assert form_of(e) in m.FORMS, e
                seen.update((form_of(e), p) for p in ctx.places(e["q"]))
                staged = e["records"] == "host" and e["table"] in rank
                if staged and prev is not None:
                    k = [len(m.records_of(x)[1]) for x in (prev, e)]
                    shrinks += k[1] < k[0] and rank[e["table"]] < rank[prev["table"]]
                    grows += k[1] > k[0] and rank[e["table"]] > rank[prev["table"]]
                prev = e if staged else None
            elif e.get("on") != "eng2":
                prev = None
    empty = []
    for f in m.FORMS:
        for name, values in CLASSES:
            for v in (OTHERS[f[0]] if values is None else values):
                key = (name,) + (v if isinstance(v, tuple) else (v,))
                if (f, key) not in seen:
                    empty.append((f, key))
    print(f"\nquery sequences, {len(m.SEEDS)} seeds x {N_STEPS} steps: {len(m.FORMS)} forms x {len(seen) // len(m.FORMS)} places; "
          f"a smaller host staging directly behind a larger one {shrinks} times, a larger behind a smaller {grows} times")
    assert not empty, f"{len(empty)} empty classes, the first: {empty[:10]}"
    assert shrinks >= 3 and grows >= 3, (shrinks, grows)


def test_census_of_the_answers():
    """Over all seeds, by what the model says is answered: every `own` table form behind a pass run with cut points off (the table is
    whole there: include/raft_hip_frag.h), and fragment_overlaps over live tensors whose records pair two reads (the sets run with
    symmetric_mode = 1 pair every read with itself, which counts no side)."""
    cuts_off = {f: 0 for f in m.FORMS if f[0] in m.TABLE_QUERIES and f[2] == "own"}
    live_pairs = 0
    for s in m.SEEDS:
        for ctx, e in walk(m.generate_with_queries(s)):
            if e["op"] != "query" or e.get("on") == "eng2" or m.outcome(ctx, e) != ("ok", None):
                continue
            if form_of(e) in cuts_off and ctx.done is not None and not ctx.done["cuts"]:
                cuts_off[form_of(e)] += 1
            if e["q"] == "fragment_overlaps" and e["records"] == "live" and not e["symmetric"] and (e["k"] is None or e["k"] >= 257):
                cols = m.records_of(e)
                live_pairs += bool((cols[1] != cols[4]).any())
    print(f"\nown tables behind a pass without cut points: {cuts_off}; fragment_overlaps over live records of two reads: {live_pairs}")
    assert all(n >= MIN_PER_CLASS for n in cuts_off.values()) and live_pairs >= MIN_PER_CLASS, (cuts_off, live_pairs)


def test_the_menus_reach_every_entry_and_every_outcome():
    qs = [(ctx_outcome, e) for s in m.SEEDS for ctx, e in walk(m.generate_with_queries(s)) if e["op"] == "query"
          for ctx_outcome in [m.outcome(ctx, e)]]
    rec = [e for _, e in qs if e["records"] != "pass"]
    assert {e["k"] for e in rec} == set(m.K_MENU) and {e["shift"] for e in rec} == {False, True}
    assert {e["table"] for e in rec} == {"none", "own", "given", "given_large"}
    assert any(e["no_target"] for e in rec if e["q"] == "repeat_overlaps") and any(e["no_target"] for e in rec if e["q"] == "repeat_stats")
    assert {e["threshold"] for _, e in qs if e["q"] == "read_stats"} == set(m.THRESHOLDS)
    assert {e["threshold"] for _, e in qs if e["q"] == "repeat_stats"} == set(m.THRESHOLDS) | {0}
    assert {e["low_cov"] for _, e in qs if e["q"] == "low_coverage"} == set(m.LOW_COV)
    assert {e["min_anchor"] for _, e in qs if e["q"] == "repeat_overlaps"} == set(m.MIN_ANCHOR)
    for q in m.QUERIES:
        got = {o for o, e in qs if e["q"] == q and e.get("on") != "eng2"}
        want = {("ok", None)} if q == "census" else {("ok", None), ("either", m.ERR_STATE)}     # (a sure ERR_STATE: on the lent engine, below)
        if q in m.TABLE_QUERIES:
            want.add(("error", m.ERR_PARAM))
        assert got == want, (q, got)
        on2 = {o for o, e in qs if e["q"] == q and e.get("on") == "eng2"}
        assert on2 == ({("ok", None)} if q == "census" else {("error", m.ERR_STATE)} if q in m.QUERIES[:3] else {("ok", None), ("error", m.ERR_STATE)}), (q, on2)


def _named_rows_agree(q, done, before):
    """Do the two passes' tables agree in every row of the reads that the (cut) stream of a repeat_overlaps call names?  That query
    looks at the runs of those reads only; the other two report every row of the table and are never excused here."""
    if q["q"] != "repeat_overlaps":
        return False
    cols = m.records_of(q)
    reads = np.unique(np.concatenate([cols[1], cols[4]]))
    (o1, s1, e1), (o2, s2, e2) = (m.tables_of(dict(q, table="own"), d)[0] for d in (done, before))
    return all(np.array_equal(s1[o1[r]:o1[r + 1]], s2[o2[r]:o2[r + 1]]) and np.array_equal(e1[o1[r]:o1[r + 1]], e2[o2[r]:o2[r + 1]]) for r in reads)


def _pass_arrays(done, keys, q):
    """The arrays of a pass named by query_sequence_model.reads_of_pass; of the coverage low_coverage sees only which windows are low
    (detect and detect_broken, whose coverage differs by the factor two, have the same empty windows)."""
    w = m.want_of(done["set"], done["variant"])
    cov = (lambda c: c <= q["low_cov"]) if q["q"] == "low_coverage" else (lambda c: c)
    return [m.columns(done["set"])["read_len"] if k == "read_len" else cov(w[k]) if k == "cov" else w[k] for k in keys]


def test_a_stale_answer_would_show():
    """Behind every change of the finished pass (set or variant), every query that reads the pass has an expected answer other than the
    one the pass before would have given to the same call.  Two exceptions, counted and printed: the two passes agree in every array the
    query reads (the histogram across runs_a / runs_sw, whose coverage is the same by construction, or across variants that move no
    window; the annotation of the many sets of the pool that have no repeat under any variant) -- there no stale read exists to be told
    apart --, and calls over a stream cut to its first k records that cannot see the difference: repeat_overlaps where the two
    annotations agree in every run of the reads the records name, and any cut between runs_a and runs_sw, whose tables differ by one
    base in the last row of some reads (only the whole stream is required to tell)."""
    told = {q: 0 for q in m.QUERIES if q != "census"}
    blind = {}
    for s in m.SEEDS:
        cur = before = None
        for ctx, e in walk(m.generate_with_queries(s)):
            done = ctx.done
            if done is not None and (cur is None or (done["set"], done["variant"]) != (cur["set"], cur["variant"])):
                before, cur = cur, done
            if e["op"] != "query" or e.get("on") == "eng2" or not m.needs_pass(e) or m.outcome(ctx, e) != ("ok", None) or before is None or done is None:
                continue
            if e["table"] == "given" and e["set"] == done["set"]:     # (`given` is another table over the same reads)
                t = e["q"] == "fragment_overlaps"
                given, own = m.tables_of(e, done)[t], m.tables_of(dict(e, table="own"), done)[t]
                fixed = all(np.array_equal(m.want_of(e["set"], v)[k], m.want_of(e["set"], 0)[k]) for v in range(len(PARAM_VARIANTS)) for k in ("rep_s", "rep_e"))
                assert any(not np.array_equal(x, y) for x, y in zip(given, own)) or (not t and fixed), e    # (most sets have one annotation under every variant: none)
            if e["records"] != "pass" and m.n_reads_of(e["set"]) != m.n_reads_of(before["set"]):
                told[e["q"]] += 1                                     # (the earlier pass would have refused the call)
                continue
            t = m.threshold_of(e, done, ctx.variant) if "threshold" in e else None
            now, then = m.expected(e, done, threshold=t), m.expected(e, before, threshold=t)
            keys = m.reads_of_pass(e)
            if e["q"] == "repeat_stats" and m.tables_of(e, done)[0][1].size == 0 and m.tables_of(e, before)[0][1].size == 0:
                keys = tuple(k for k in keys if not k.startswith("cov"))      # (no run in either table: no window is looked at)
            if m.differ(e, then, now):
                told[e["q"]] += 1
                continue
            same = all(np.array_equal(x, y) for x, y in zip(_pass_arrays(done, keys, e), _pass_arrays(before, keys, e)))
            few = e["records"] != "pass" and e["k"] is not None and ({before["set"], done["set"]} == {"runs_a", "runs_sw"} or
                                                                       _named_rows_agree(e, done, before))
            assert same or few, f"seed {s}: {e} answers the same behind {before} and {done}, which differ in {keys}"
            why = (e["q"],) + (("the passes agree in",) + keys if same else ("a cut stream",))
            blind[why] = blind.get(why, 0) + 1
    print(f"\nstale answers that would show: {told}; pairs of passes equal in all a query reads: {blind}")
    assert all(n >= 5 for n in told.values()), told


# ---- the fast sibling of repeat_stats_model ------------------------------------------------------------------------------------------------
def _model_cases():
    cols, rep = rst_cases.lattice_case()
    off, cov = rst_cases.synthetic_coverage(cols[0], 50)
    covered = dict(threshold=20, cov_offset=off, cov=cov, reso=50)
    for sym in (False, True):
        yield f"lattice_case, symmetric {sym}", cols, sym, rep, {}
        yield f"lattice_case with coverage, symmetric {sym}", cols, sym, rep, covered
        for n in (0, 1, 257, 5000):
            c, r = rst_cases.stream(n)
            yield f"stream({n}), symmetric {sym}", c, sym, r, covered
        c, r = rst_cases.stream(257)
        yield f"stream(257) without ts / te, symmetric {sym}", c[:5] + [None, None], True, r, {}
    for n in rst_cases.STREAKS[:-1]:
        for column in "qt":
            c, r = rst_cases.streak_case(n, column)
            yield f"streak_case({n}, {column})", c, False, r, {}
    yield "no records", [cols[0]] + [None] * 6, False, rep, covered


def test_the_fast_sibling_equals_the_model_on_the_models_cases():
    for what, cols, sym, rep, kw in _model_cases():
        rst_cases.same_stats(m.repeat_stats_fast(*cols, sym, *rep, **kw), rst_cases.repeat_stats_model(*cols, sym, *rep, **kw), what)


@pytest.mark.parametrize("mistake", rst_cases.MISTAKES)
def test_the_fast_sibling_catches_the_models_planted_mistakes(mistake):
    (cols, sym, rep, kw), what = rst_cases._mistake_case(mistake)
    fast = m.repeat_stats_fast(*cols, sym, *rep, **kw)
    rst_cases.same_stats(fast, rst_cases.repeat_stats_model(*cols, sym, *rep, **kw), what)
    with pytest.raises(AssertionError):
        rst_cases.same_stats(rst_cases.repeat_stats_model(*cols, sym, *rep, mistake=mistake, **kw), fast, f"{what}, with {mistake}")


def _ovl_cases():
    for name in sorted(ovl_cases.HAND):
        cols, sym, anchor, rep, _ = ovl_cases.hand_case(name)
        yield name, cols, sym, anchor, rep
    for n in (0, 1, 5, 257, 1025, 5000):
        cols, rep = ovl_cases.stream(n)
        for sym, anchor in ((False, 300), (True, 1)):
            yield f"stream({n})", cols, sym, anchor, rep
    for name, anchor in ovl_cases.GOLDEN_ANCHORS.items():
        cols, rep = ovl_cases.golden_case(name)
        yield name, cols, False, anchor, rep
    lens, runs = rst_cases.case_reads()                      # (runs tied at start 0, an EMPTY run, runs outside the read)
    cols, _ = rst_cases.stream(1025)
    yield "the reads of the repeat_stats cases", cols, False, 100, rst_cases.csr(runs)


def test_the_fast_side_share_equals_the_models_on_the_models_cases():
    for what, cols, sym, anchor, rep in _ovl_cases():
        n = len(cols[0])
        for rid, a, b in ((cols[1], cols[2], cols[3]), (cols[4], cols[5], cols[6])):
            assert np.array_equal(m.side_rep_fast(n, rid, a, b, *rep), ovl_cases._side_rep(n, rid, a, b, *[np.asarray(x, np.int64) for x in rep])), what
        before = m.fast_calls[0]
        fast = m.want_classes_fast(*cols, sym, anchor, *rep)
        assert m.fast_calls[0] > before, "want_classes_fast did not go through side_rep_fast"
        before = m.fast_calls[0]
        ovl_cases.same_classes(fast, ovl_cases.want_classes(*cols, sym, anchor, *rep), what)
        assert m.fast_calls[0] == before, "want_classes went through side_rep_fast"
    assert ovl_cases._side_rep is not m.side_rep_fast


def test_the_large_table_is_larger_than_any_oracle_table():
    for s in m.SEEDS:
        for ctx, e in walk(m.generate_with_queries(s)):
            if e["op"] == "query" and e["table"] == "given_large":
                rows = m.large_table(m.n_reads_of(e["set"]))[1].size
                w = m.want_of(e["set"], m.given_variant(e["set"], e["avoid"], False))
                assert rows > max(w["rep_s"].size, w["frag_begin"].size), (e, rows)


def test_model_cost_of_one_seed():
    m.want_of("runs_a", 0)                     # (the oracle is built and loaded)
    m._expected.clear(); m.plain._wants.clear()
    t = time.perf_counter()
    n = 0
    for ctx, e in walk(m.generate_with_queries(0)):
        if e["op"] == "query" and m.outcome(ctx, e) == ("ok", None):
            m.expected(e, ctx.held(), ctx.variant)
            n += 1
    print(f"\nthe expected answers of seed 0 from a cold cache: {n} queries, {time.perf_counter() - t:.2f} s")
