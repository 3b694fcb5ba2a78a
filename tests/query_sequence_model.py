"""The post-pass queries inside call sequences on ONE engine context: the op lists, the model of the context and the expected answers
behind tests/test_gpu_query_sequences.py.

generate_with_queries(seed, n_steps) is context_model.generate(seed, n_steps) unchanged, with 0 to 3 query ops behind every op (setting
changes and pipelined jobs too).  A query op names the query, its form -- whose records (`live`: the caller's device tensors of the last
run_device, `host`: numpy columns of a set), whose table (`own`: the finished pass, `given`: the oracle's tables of the records' set under
ANOTHER parameter variant, `given_large`: more rows than any oracle table) -- and its arguments from small fixed menus, so that the
expected answers memoise by (records, last finished pass, op).  How many queries follow an op and their arguments come from a
random.Random of their own; WHICH form comes next is the one with the most classes of the census still empty (test_query_sequence_model.py
CLASSES) in the place it would land, over the seeds in order -- still a function of the seed alone.

Context is the model of what a query must return: the finished pass the context holds (set, variant, width, cut points) or none (before
the first pass); behind a host-to-host job it holds none or, where the job was served in one piece, the job's
(outcome()).  Expected answers come from the numpy models of the queries' own test files, fed with the
oracle's result for the set and variant of the LAST FINISHED pass, never from anything the library returns.

Plain Python and numpy: imports and runs without a GPU."""
from __future__ import annotations

import random

import numpy as np
import test_fragment_overlaps_cases as frag_cases
import test_repeat_overlaps_cases as ovl_cases
import test_repeat_stats_cases as rst_cases
from context_model import N_STEPS, PARAM_VARIANTS, PASS_OPS, SETS, generate, params_of
import test_gpu_context_sequences as plain
from test_gpu_census import want_census
from test_gpu_cov_hist import want_hist
from test_gpu_read_stats import want_stats
from test_low_cov_cases import same_low, want_low

# the seeds of test_gpu_context_sequences.py (the flag lists are compared seed by seed): 12 fill the census of the op lists, the GPU
# file's census of answers per path needs all 16
SEEDS = tuple(range(16))
QUERIES = ("coverage_histogram", "read_stats", "low_coverage", "census", "repeat_overlaps", "fragment_overlaps", "repeat_stats")
TABLE_QUERIES = QUERIES[4:]
# (query, records, table): every form a query has here
FORMS = (tuple((q, "pass", "own") for q in QUERIES[:3]) + (("census", "live", "none"), ("census", "host", "none")) +
         tuple((q, r, t) for q in TABLE_QUERIES for r in ("live", "host") for t in ("own", "given")))
K_MENU = (0, 1, 5, 257, 1025, None)           # the first k records (None: all): nothing, one, a lane and one, a wave and one, a workgroup and one
K_WEIGHTS = (2, 2, 3, 3, 3, 1)
THRESHOLDS = (1, 5, "high", None)             # "high": the high_cov of the last finished pass; None: the context's, at the call
LOW_COV = (0, 3, 300, 70000)                  # both sides of the byte and the two-byte code limits (test_gpu_query_staging.LOW_COV)
MIN_ANCHOR = (0, 300, 1000)                  # 0 is refused: min_anchor < 1 -> ERR_PARAM in any state
PERMILLE = 800
RESO = 50
# `given`: the first of these variants, other than the pass's, under which the set's table differs from the pass's (fragment tables:
# read_length moves every one; annotations: repeat_length, est_cov, the flanks -- for the sets that have a repeat at all)
GIVEN_VARIANTS = {True: (4, 0), False: (len(PARAM_VARIANTS) - 1, 1, 3, 0)}
SETTINGS = ("width", "cuts", "params_keep", "params_minbins")
ERR_PARAM, ERR_STATE = 1, 7                   # raft_amd.engine's codes (the GPU test checks they are)
# the name a query's refusal carries in the context's message (raft_hip_last_error)
MESSAGE_NAME = {"coverage_histogram": "raft_hip_cov_histogram", "read_stats": "raft_hip_read_stats", "low_coverage": "raft_hip_low_coverage",
                "census": "census", "repeat_overlaps": "repeat_overlaps", "fragment_overlaps": "fragment_overlaps", "repeat_stats": "repeat_stats"}
COLS = ("read_len", "qid", "qs", "qe", "tid", "ts", "te")


# ---- the model of the context -------------------------------------------------------------------------------------------------------------
class Context:
    """What the ops before a query leave on the context, as far as a query can tell: `done` = the finished pass it holds (set, variant,
    width, cuts) or None; `content` = the set in the caller's device tensors; the settings for the next pass; and where the query lands
    (the last pass op, the op directly before, the settings changed since the last pass) for the census."""

    def __init__(self):
        self.content = None
        self.variant, self.width, self.cuts = 0, 4, True
        self.done = None
        self.job, self.jobs = None, 0          # the host-to-host job since the last finished pass: {"set", "variant", "n": which}
        self.last_pass = None                  # the last pass op (pipelined jobs too), with the width it ran under
        self.changed = set()
        self.prev = None

    def apply(self, e):
        op = e["op"]
        if op == "query":
            self.prev = e
            return
        if op in ("copy", "alias", "new", "targets"):
            self.content = e["set"]
        if op in ("same", "copy", "alias", "new", "targets") or (op == "outputs_edit" and self.done is not None):
            self._finished(e, self.content)
        elif op in ("host", "host_grouped", "windows"):
            self._finished(e, e["set"])
        elif op in ("pipelined1", "pipelined2"):
            self.done = None
            self.jobs += 1
            # a job of one chunk is served in one piece (engine_pipeline.hip plan_chunks: fewer than two chunks; choose_route: the
            # host-routed path needs several contexts or chunks) -- but for two contexts over a stream that is not symmetric
            one_piece = e["chunks"] == 1 and (op == "pipelined1" or SETS[e["set"]][1] == 1)
            self.job = {"set": e["set"], "variant": self.variant, "n": self.jobs, "one_piece": one_piece}
            self.last_pass = dict(e, width=None)
            self.changed = set()
        elif op in ("params_keep", "params_minbins"):
            self.variant = e["variant"]
        elif op == "width":
            self.width = e["width"]
        elif op == "cuts":
            self.cuts = e["on"]
        if op in SETTINGS:
            self.changed.add(op)
        self.prev = e

    def _finished(self, e, name):
        self.done = {"set": name, "variant": self.variant, "width": self.width, "cuts": self.cuts}
        self.job = None
        self.last_pass = dict(e, width=self.width, set=name)
        self.changed = set()

    def held(self):
        """The pass a query reads here for sure: the finished one, or that of a job served in one piece; else None."""
        return self.done if self.done is not None else self.job if self.job is not None and self.job["one_piece"] else None

    def pass_set(self):
        """The set of the last pass op, finished or not: what a host form takes its columns from."""
        return None if self.last_pass is None else self.last_pass["set"]

    def places(self, query):
        """The classes of the census a query of this kind would fall into here."""
        out = []
        lp = self.last_pass
        if lp is not None:
            if lp["op"] in PASS_OPS:
                out.append(("kind", lp["op"]))
            if lp["op"].startswith("pipelined"):
                out.append(("pipelined",))
            else:
                out.append(("width", lp["width"]))
        p = self.prev
        if p is not None and p["op"] == "query" and p.get("on") != "eng2" and p["q"] != query:
            out.append(("after", p["q"]))
        if p is not None and p["op"] in PASS_OPS and not p["op"].startswith("pipelined"):
            if p["route"] == "fetch":
                out.append(("route", "fetch"))
            elif p["route"] in ("fetch_packed", "fetch_delta4"):
                out.append(("route", "packed"))
        out += [("setting", s) for s in sorted(self.changed)]
        return out


def needs_pass(q) -> bool:
    """Does this query op read the context's finished pass (its coverage or one of its tables)?"""
    return q["table"] == "own" or (q["q"] == "repeat_stats" and q["threshold"] != 0)


def n_reads_of(name) -> int:
    return int(columns(name)["read_len"].size)


def outcome(ctx: Context, q):
    """("ok", None) or ("error", code): what the headers promise for this query in this state of the context.  ("either", ERR_STATE)
    behind a host-to-host job: a job cut into chunks leaves no pass (ERR_STATE), one that the library served in one piece leaves its
    pass on the first context as raft_hip_run_host + raft_hip_finish would (include/raft_hip.h; tests/test_gpu_pipeline_edges.py
    check_route).  A job of one chunk is one piece for sure (Context.apply) and its pass is expected like any other; for the others
    the route is the planner's decision (tests/pipeline_cases.py models it), not this model's: the query is refused with ERR_STATE,
    or answers for the job's pass (ctx.job), or refuses another number of reads with ERR_PARAM -- and every query behind one job
    sees the same of the two states."""
    if q["q"] == "repeat_overlaps" and q["min_anchor"] < 1:      # (include/raft_hip_ovl.h: checked before the state)
        return ("error", ERR_PARAM)
    if q.get("on") == "eng2":                  # the second engine of a pipelined2 job: lent, never holds a pass
        return ("error", ERR_STATE) if needs_pass(q) else ("ok", None)
    if not needs_pass(q):
        return ("ok", None)
    held = ctx.held()
    if held is None and ctx.job is not None:
        return ("either", ERR_STATE)
    if held is None:
        return ("error", ERR_STATE)
    if q["records"] != "pass" and n_reads_of(q["set"]) != n_reads_of(held["set"]):
        return ("error", ERR_PARAM)
    return ("ok", None)


# ---- the op lists --------------------------------------------------------------------------------------------------------------------------
def _draw_args(rng, ctx, form, force=None):
    name, records, table = form
    q = {"op": "query", "q": name, "records": records, "table": table}
    if records != "pass":
        q["set"] = ctx.content if records == "live" or rng.random() < 0.3 or ctx.pass_set() is None else ctx.pass_set()
        if q["set"] is None:                   # (before the first pass there are no tensors: a host form over the first set's group)
            q["records"], q["set"] = "host", "runs_a"
        q["k"] = rng.choices(K_MENU, weights=K_WEIGHTS)[0]
        q["shift"] = rng.random() < 0.2
        q["symmetric"] = SETS[q["set"]][1] == 1
        q["no_target"] = bool(q["symmetric"] and name != "fragment_overlaps" and (name == "census" or rng.random() < 0.4))
        if name == "fragment_overlaps" and q["records"] == "host" and q["symmetric"]:
            q["partnered"] = True
    if table != "none" and records != "pass":
        q["avoid"] = ctx.held()["variant"] if ctx.held() is not None else ctx.variant  # the variant `given` must not be: the pass's
        if table == "given" and name != "fragment_overlaps" and rng.random() < 0.25:
            q["table"] = "given_large"
    if name == "read_stats":
        q["threshold"] = rng.choice(THRESHOLDS)
    elif name == "repeat_stats":
        q["threshold"] = rng.choice((0,) + THRESHOLDS) if table != "own" or rng.random() < 0.5 else rng.choice(THRESHOLDS)
    elif name == "low_coverage":
        q["low_cov"] = rng.choice(LOW_COV)
    elif name == "repeat_overlaps":
        q["min_anchor"] = rng.choice(MIN_ANCHOR)
    if force:
        q.update(force)
    return q


def _pick_form(rng, ctx, seen):
    best, forms = -1, []
    for f in FORMS:
        n = sum((f, p) not in seen for p in ctx.places(f[0]))
        if n > best:
            best, forms = n, []
        if n == best:
            forms.append(f)
    name = rng.choice(sorted({f[0] for f in forms}))            # (every query alike, however many forms it has)
    return rng.choice([f for f in forms if f[0] == name])


def _generate(seed, n_steps, seen):
    rng = random.Random(1_000_003 * seed + 17)
    ctx = Context()
    out = []

    def add(q):
        for p in ctx.places(q["q"]):
            seen.add(((q["q"], q["records"], "given" if q["table"] == "given_large" else q["table"]), p))
        out.append(q)
        ctx.apply(q)

    for e in generate(seed, n_steps):
        out.append(e)
        ctx.apply(e)
        if e["op"] == "pipelined2":           # the engine the job borrowed: no pass of its own, so own forms are refused and the others answer
            for form, extra in ((("coverage_histogram", "pass", "own"), {}), (("read_stats", "pass", "own"), {"threshold": 5}),
                                (("low_coverage", "pass", "own"), {"low_cov": 3}), (("census", "host", "none"), {}),
                                (("repeat_overlaps", "host", "own"), {"min_anchor": 300}), (("repeat_overlaps", "host", "given"), {"min_anchor": 300}),
                                (("fragment_overlaps", "host", "own"), {}), (("fragment_overlaps", "host", "given"), {}),
                                (("repeat_stats", "host", "given"), {"threshold": 0}), (("repeat_stats", "host", "given"), {"threshold": 5})):
                q = _draw_args(rng, ctx, form, dict(extra, on="eng2", records=form[1], set=e["set"], symmetric=SETS[e["set"]][1] == 1))
                if form[1] != "pass" and q["k"] is None:
                    q["k"] = 1025
                q["no_target"] = bool(q.get("no_target") and q["symmetric"])
                out.append(q)                  # (not part of the census, and not `prev` of what follows on the first engine)
        n = rng.choice((0, 1, 1, 2, 2, 3))
        pair = n >= 2 and rng.random() < 0.25
        first_big = rng.random() < 0.5
        for j in range(n):
            form = _pick_form(rng, ctx, seen)
            force = None
            if pair and j < 2:                 # a larger staging directly before a smaller one, and the other way round
                big = first_big == (j == 0)
                form = ("repeat_stats", "host", "given") if big else (rng.choice(TABLE_QUERIES), "host", "given")
                force = {"k": rng.choice((1025, None)) if big else rng.choice((0, 1, 5)), "table": "given_large" if big else "given"}
            add(_draw_args(rng, ctx, form, force))
    return out


_lists: dict = {}
_seen: set = set()


def generate_with_queries(seed: int, n_steps: int = N_STEPS) -> list[dict]:
    """The op list of a seed.  For the seeds and the length the GPU test runs, the lists are made in seed order, each choosing its forms
    by what the lists before it left empty; any other (seed, n_steps) is made on its own.  Deterministic either way."""
    if seed in SEEDS and n_steps == N_STEPS:
        if not _lists:
            for s in SEEDS:
                _lists[s] = _generate(s, N_STEPS, _seen)
        return [dict(e) for e in _lists[seed]]
    return _generate(seed, n_steps, set())


def pass_ops(ops):
    return [e for e in ops if e["op"] != "query"]


# ---- the inputs ----------------------------------------------------------------------------------------------------------------------------
_large: dict = {}


def columns(name):
    return plain._set(name)


def want_of(name, variant):
    """The oracle's result for a set under a parameter variant, shared with test_gpu_context_sequences.py (which imports without a GPU)."""
    return plain._want(name, variant)


def high_cov_at_call(variant) -> int:
    """The default threshold of read_stats and repeat_stats as Engine's docstrings give it: int(est_cov * cov_mul) of the parameters in force."""
    p = params_of(variant, 1)
    return int(p.est_cov * p.cov_mul)


def large_table(n_reads):
    """A table with more rows than any oracle table of the pool: 130 runs on every eighth read (test_repeat_stats_cases.R_130's), none on
    the others.  Valid as an annotation and as a fragment table."""
    if n_reads not in _large:
        runs = rst_cases.case_reads()[1][rst_cases.R_130]
        _large[n_reads] = rst_cases.csr([runs if r % 8 == 0 else [] for r in range(n_reads)])
    return _large[n_reads]


def given_variant(name, avoid, fragments: bool) -> int:
    keys = ("frag_offset", "frag_begin", "frag_end") if fragments else ("rep_offset", "rep_s", "rep_e")
    own = want_of(name, avoid)
    others = [v for v in GIVEN_VARIANTS[fragments] if v != avoid]
    for v in others:
        if any(not np.array_equal(want_of(name, v)[k], own[k]) for k in keys):
            return v
    return others[0]


_partnered: dict = {}
PARTNER = 997


def partnered(name):
    """A symmetric set's columns with every record's target side taken from the record PARTNER places on: the sets run with
    symmetric_mode = 1 repeat the query columns as targets, and a record of a read with itself counts no side in fragment_overlaps."""
    if name not in _partnered:
        c = dict(columns(name))
        for t, k in (("tid", "qid"), ("ts", "qs"), ("te", "qe")):
            c[t] = np.ascontiguousarray(np.roll(c[k], -PARTNER))
        _partnered[name] = c
    return _partnered[name]


def records_of(q, source=None):
    """The seven columns of a query op: read_len whole, the record columns cut to k records, from one element in when `shift`, ts / te
    None when `no_target`.  `source`: the caller's tensors for the live form (default: the set's numpy columns)."""
    c = source if source is not None else partnered(q["set"]) if q.get("partnered") else columns(q["set"])
    a = 1 if q["shift"] else 0
    b = None if q["k"] is None else a + q["k"]
    cols = [c["read_len"]] + [c[k][a:b] for k in COLS[1:]]
    if q["no_target"]:
        cols[5] = cols[6] = None
    return cols


def tables_of(q, done):
    """-> (repeats, fragments) as numpy CSR triples: the pass's for `own`, the other variant's or the large table for `given`."""
    if q["table"] == "own":
        w = want_of(done["set"], done["variant"])
    elif q["table"] == "given_large":
        t = large_table(n_reads_of(q["set"]))
        return t, t
    else:
        w = want_of(q["set"], given_variant(q["set"], q["avoid"], q["q"] == "fragment_overlaps"))
    return (w["rep_offset"], w["rep_s"], w["rep_e"]), (w["frag_offset"], w["frag_begin"], w["frag_end"])


def threshold_of(q, done, variant_now) -> int:
    t = q["threshold"]
    if t is None:
        return high_cov_at_call(variant_now)
    if t == "high":
        return max(int(want_of(done["set"], done["variant"])["high_cov"]), 1) if done is not None else 5
    return t


# ---- the expected answers ------------------------------------------------------------------------------------------------------------------
def repeat_stats_fast(read_len, qid, qs, qe, tid, ts, te, symmetric, rep_offset, rep_s, rep_e, threshold=0, cov_offset=None, cov=None, reso=None):
    """test_repeat_stats_cases.repeat_stats_model with the sides grouped by read ONCE (one sort) and the window ranges reduced in one
    sweep: the same definitions of include/raft_hip_rst.h, for 3000 reads x 120,000 sides.  test_query_sequence_model.py shows it equal
    to that model on the model's own cases."""
    L = np.asarray(read_len, np.int64)
    off, S, E = np.asarray(rep_offset, np.int64), np.asarray(rep_s, np.int64), np.asarray(rep_e, np.int64)
    n_reads, n_rep = len(L), len(S)
    if qid is None:
        rid = a = b = np.zeros(0, np.int64)
    else:
        rid, a, b = rst_cases.counted_sides(qid, qs, qe, tid, ts, te, symmetric)
    real = b > a
    order = np.argsort(rid[real], kind="stable")
    rid, a, b = rid[real][order], a[real][order], b[real][order]
    first = np.searchsorted(rid, np.arange(n_reads + 1), side="left")
    run_read = np.repeat(np.arange(n_reads), np.diff(off))
    out = {k: np.zeros(n_rep, np.int32) for k in rst_cases.COUNTS}
    out["run_flags"] = (np.where(E <= S, rst_cases.EMPTY, 0) | np.where(S <= 0, rst_cases.AT_START, 0) |
                        np.where(E >= L[run_read], rst_cases.AT_END, 0)).astype(np.uint8) if n_rep else np.zeros(0, np.uint8)
    for r in np.flatnonzero((np.diff(off) > 0) & (np.diff(first) > 0)):
        k = np.arange(off[r], off[r + 1])
        k = k[E[k] > S[k]]
        x, y = a[first[r]:first[r + 1]][None, :], b[first[r]:first[r + 1]][None, :]
        s, e = S[k][:, None], E[k][:, None]
        out["run_touch"][k] = ((x < e) & (y > s)).sum(axis=1)
        out["run_span"][k] = ((x <= s) & (y >= e)).sum(axis=1)
        out["run_inside"][k] = ((x >= s) & (y <= e)).sum(axis=1)
    for k in rst_cases.COVERAGE:
        out[k] = None
    if threshold >= 1:
        cov_offset, cov = np.asarray(cov_offset, np.int64), np.asarray(cov, np.int64)
        W = np.diff(cov_offset)[run_read]
        j0 = np.maximum(S, 0) // reso
        j1 = np.minimum(-(-E // reso), W)
        n = np.where(E <= S, 0, np.maximum(j1 - j0, 0))
        out.update({k: np.zeros(n_rep, np.int64 if k == "run_cov_sum" else np.int32) for k in rst_cases.COVERAGE})
        out["run_windows"] = n.astype(np.int32)
        some = np.flatnonzero(n > 0)
        if some.size:
            lo = cov_offset[run_read[some]] + j0[some]
            hi = lo + n[some]
            cs = np.concatenate([[0], np.cumsum(cov)])
            ch = np.concatenate([[0], np.cumsum(cov >= threshold)])
            out["run_cov_sum"][some] = cs[hi] - cs[lo]
            out["run_high"][some] = ch[hi] - ch[lo]
            padded = np.concatenate([cov, [0]])                     # (so that a range may end at the array's end)
            idx = np.stack([lo, hi], axis=1).reshape(-1)
            out["run_cov_min"][some] = np.minimum.reduceat(padded, idx)[::2]
            out["run_cov_max"][some] = np.maximum.reduceat(padded, idx)[::2]
    f = out["run_flags"]
    out.update(n_runs=n_rep, runs_empty=int((f & rst_cases.EMPTY != 0).sum()), runs_interior=int((f == 0).sum()),
               runs_touched=int((out["run_touch"] > 0).sum()), runs_spanned=int((out["run_span"] > 0).sum()),
               interior_spanned=int(((f == 0) & (out["run_span"] > 0)).sum()), sides_touch=int(out["run_touch"].astype(np.int64).sum()),
               sides_span=int(out["run_span"].astype(np.int64).sum()), sides_inside=int(out["run_inside"].astype(np.int64).sum()),
               windows=0 if threshold < 1 else int(out["run_windows"].astype(np.int64).sum()), cov_sum=0 if threshold < 1 else int(out["run_cov_sum"].sum()))
    return out


fast_calls = [0]          # calls of side_rep_fast (the CPU test checks that want_classes_fast really goes through it)


def side_rep_fast(n_reads, rid, a, b, rep_offset, rep_s, rep_e):
    """test_repeat_overlaps_cases._side_rep -- |[a, b) intersected with U(read)| for every side -- without a Python loop over the reads:
    the disjoint pieces of all reads from ONE sort and a running maximum, a side's share from two searches in the pieces' prefix sums."""
    fast_calls[0] += 1
    off, S, E = np.asarray(rep_offset, np.int64), np.asarray(rep_s, np.int64), np.asarray(rep_e, np.int64)
    a, b, rid = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64), np.asarray(rid).astype(np.int64)
    R = np.repeat(np.arange(n_reads, dtype=np.int64), np.diff(off))
    real = E > S
    R, S, E = R[real], S[real], E[real]
    if S.size == 0 or a.size == 0:
        return np.zeros(a.shape, np.int64)
    BIG = np.int64(1) << 33                                             # more than any difference of two int32 coordinates
    order = np.lexsort((E, S, R))
    R, S, E = R[order], S[order], E[order]
    top = np.maximum.accumulate(E + R * BIG) - R * BIG                  # the furthest end so far within the read
    first = np.ones(S.size, bool)
    first[1:] = (R[1:] != R[:-1]) | (S[1:] > top[:-1])                  # (a run that only touches the piece before it joins it)
    piece = np.cumsum(first) - 1
    pr, ps = R[first], S[first]
    pe = np.zeros(ps.size, np.int64)
    np.maximum.at(pe, piece, E)
    below = np.concatenate([[0], np.cumsum(pe - ps)])                   # the bases of all pieces before piece j
    base = np.searchsorted(pr, rid, side="left")

    def covered(x):                                                     # the bases of U(read) below x
        j = np.searchsorted(pr * BIG + ps, rid * BIG + x, side="left")  # the pieces of the read (and of the reads before it) that begin below x
        last = np.maximum(j - 1, 0)
        part = np.minimum(x, pe[last]) - ps[last]
        return np.where(j > base, below[last] - below[base] + part, 0)
    return np.maximum(covered(b) - covered(a), 0)


def want_classes_fast(*args):
    """test_repeat_overlaps_cases.want_classes with side_rep_fast in the place of its _side_rep (the rest is that model's own code);
    test_query_sequence_model.py shows the two equal on that model's hand-written, generated and golden cases."""
    slow = ovl_cases._side_rep
    ovl_cases._side_rep = side_rep_fast
    try:
        return ovl_cases.want_classes(*args)
    finally:
        ovl_cases._side_rep = slow


def _freeze(q, done, threshold):
    key = tuple(sorted((k, v) for k, v in q.items() if k not in ("op", "on", "threshold")))
    return key, None if done is None else (done["set"], done["variant"]), threshold


_expected: dict = {}


def expected(q, done, variant_now=0, threshold=None):
    """The answer the query must give behind the finished pass `done` ({"set", "variant", ...}; None where it reads none), memoised.
    `threshold`: the number to take in place of the op's menu entry (to ask what ANOTHER pass would have answered to the same call)."""
    if threshold is None:
        threshold = threshold_of(q, done, variant_now) if "threshold" in q else None
    key = _freeze(q, done if needs_pass(q) else None, threshold)
    if key not in _expected:
        _expected[key] = _compute(q, done, threshold)
    return _expected[key]


def _compute(q, done, threshold):
    name = q["q"]
    w = want_of(done["set"], done["variant"]) if needs_pass(q) else None
    if name == "coverage_histogram":
        return want_hist(w["cov"])
    if name == "read_stats":
        return want_stats(w, threshold)
    if name == "low_coverage":
        return want_low(w, columns(done["set"])["read_len"], RESO, q["low_cov"], PERMILLE)
    cols = records_of(q)
    if name == "census":
        return want_census(*cols, q["symmetric"])
    rep, frag = tables_of(q, done)
    if name == "repeat_overlaps":
        return want_classes_fast(*cols, q["symmetric"], q["min_anchor"], *rep)
    if name == "fragment_overlaps":
        return frag_cases.want_fragments(*cols, q["symmetric"], *frag, *rep)
    cov = dict(threshold=threshold, cov_offset=w["cov_offset"], cov=w["cov"], reso=RESO) if threshold >= 1 else {}
    return repeat_stats_fast(*cols, q["symmetric"], *rep, **cov)


def reads_of_pass(q):
    """The arrays of the oracle's result this query's answer depends on (beside its own arguments): where two passes agree in all of
    them, no stale read of the one could be told from the other."""
    name = q["q"]
    if name == "coverage_histogram":
        return ("cov",)
    if name == "read_stats":
        return ("cov", "cov_offset")
    if name == "low_coverage":
        return ("cov", "cov_offset", "read_len")
    keys = ()
    if q["table"] == "own":
        keys += ("rep_offset", "rep_s", "rep_e") + (("frag_offset", "frag_begin", "frag_end") if name == "fragment_overlaps" else ())
    if name == "repeat_stats" and q["threshold"] != 0:
        keys += ("cov", "cov_offset")
    return keys


def same_answer(q, got, exp, what):
    """The comparison of the query's own GPU file, exact in every array, dtype and count."""
    name = q["q"]
    if name == "coverage_histogram":
        assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.shape == exp.shape and np.array_equal(got, exp), f"{what}: the histogram differs"
    elif name == "read_stats":
        assert got["cov_sum"].dtype == np.int64 and got["cov_max"].dtype == np.int32 and got["high_windows"].dtype == np.int32, what
        for k in ("cov_sum", "cov_max", "high_windows"):
            assert got[k].shape == exp[k].shape, (what, k, got[k].shape, exp[k].shape)
            bad = np.flatnonzero(got[k].astype(np.int64) != exp[k])
            assert bad.size == 0, f"{what}: {k} differs on {bad.size} reads, first read {bad[0]}: got {got[k][bad[0]]} want {exp[k][bad[0]]}"
    elif name == "low_coverage":
        same_low(got, exp, what)
    elif name == "census":
        wi, wf = exp
        assert got["intervals"].dtype == np.int32 and got["contained"].dtype == np.uint8, what
        assert np.array_equal(got["intervals"], wi), f"{what}: intervals differ"
        assert np.array_equal(got["contained"], wf), f"{what}: contained flags differ"
        assert got["n_contained"] == int((wf != 0).sum()), what
    elif name == "repeat_overlaps":
        ovl_cases.same_classes(got, exp, what)
    elif name == "fragment_overlaps":
        frag_cases.same_fragments(got, exp, what)
    else:
        rst_cases.same_stats(got, exp, what)


def differ(q, x, y) -> bool:
    """Would same_answer tell x from y?"""
    try:
        if q["q"] == "read_stats":
            x = {"cov_sum": x["cov_sum"], "cov_max": x["cov_max"].astype(np.int32), "high_windows": x["high_windows"].astype(np.int32)}
        elif q["q"] == "census":
            x = {"intervals": x[0].astype(np.int32), "contained": x[1], "n_contained": int((x[1] != 0).sum())}
        same_answer(q, x, y, "")
    except AssertionError:
        return True
    return False
