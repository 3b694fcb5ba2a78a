"""The cases of tests/pipeline_cases.py on the CPU: what the real planner (tests/pipeline_plan_print.cpp over raft_amd/csrc/pipeline_plan.hpp,
built by the host compiler under the address and undefined-behaviour sanitizers, a process of its own) makes of every case equals what the
plain-Python model makes of it and the case's literal claims, as plain columns and as grouped offsets; every class a case claims holds by
the model and the oracle; no class of the census is empty."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest
from pipeline_cases import CASES, CLASSES, CONTEXTS, MINBINS, ROUTED, CaseModel, case_id, holds, model_jobs, model_plan, model_routed, sampled_runs

HERE = os.path.dirname(os.path.abspath(__file__))

@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "pipeline_plan_print")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-static-libasan", "-static-libubsan", "-pthread",       # (the runtimes inside the program: nothing to load beside it)
                            os.path.join(HERE, "pipeline_plan_print.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return exe


def planned(exe, case, grouped, d4):
    """(runs | None, plan, {n_ctx: (jobs, caps)}) as the planner prints them."""
    p = case.p
    head = [p.reso, MINBINS, p.interval_length, case.n_chunks, int(d4), case.n_reads, *case.read_len.tolist()]
    body = [1, case.n_runs, case.n_rec, *case.offsets.reshape(-1).tolist()] if grouped else [0, 0, case.n_rec, *case.cols[0].tolist()]
    run = subprocess.run([exe], input=" ".join(str(int(x)) for x in head + body), capture_output=True, text=True)
    assert run.returncode == 0, (case, run.stdout[-2000:], run.stderr[-2000:])
    runs, plan, jobs = None, [], {}
    for line in run.stdout.splitlines():
        w = line.split()
        v = [int(x) for x in w[1:]]
        if w[0] == "runs":
            runs = v[1:] if v[0] >= 1 else None
        elif w[0] == "chunk":
            plan.append((v[0], v[1], tuple(v[3:]), v[2]))
        elif w[0] == "jobs":
            n_ctx = v[0]
            jobs[n_ctx] = ([], tuple(v[2:5]))
        else:
            jobs[n_ctx][0].append(tuple(v))
    return runs, plan, jobs


PAIRS = [(c, g) for c in CASES for g in (False, True) if ("grouped" if g else "columns") in c.forms]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("case,grouped", PAIRS, ids=[f"{c.name}-{'grouped' if g else 'columns'}" for c, g in PAIRS])
def test_the_planner_the_model_and_the_claims_agree(planner, case, grouped):
    for d4 in sorted({w == 8 for w in case.widths}):
        runs, plan, jobs = planned(planner, case, grouped, d4)
        what = (case, "grouped" if grouped else "columns", "delta4" if d4 else "bytes")
        # the runs: grouped, what the offsets say (five: none the plan keeps pieces for); plain columns, what the samples show
        if grouped:
            assert (runs is None) == (case.n_runs > 4), what
            if runs is not None:
                starts = [0]
                for r in case.runs:
                    starts.append(starts[-1] + len(r))
                assert runs == starts, what
        else:
            assert runs == sampled_runs(case.cols[0].tolist()), what
            assert (len(runs) - 1 if runs else None) == {"chunked": case.n_runs, "one piece": case.n_runs, "routed": None, "redo": 1}[case.route], what
        if runs is None:
            assert case.route in ("routed", "one piece") and not plan, what
            continue
        # the plan: the planner's, the model's, the claim
        if case.route == "redo":            # (the planner searches a column that is not sorted: only that it cuts the job is claimed)
            assert len(plan) >= 2 and [c[:2] for c in plan] == [c[:2] for c in case.plan], what
            continue
        model, claim = model_plan(case.read_len, case.run_ids, case.n_chunks, d4), case.plan8 if d4 else case.plan
        assert plan == model, (what, plan, model)
        assert plan == claim, (what, plan, claim)
        assert (len(plan) >= 2) == (case.route == "chunked" and case.plan_for(8 if d4 else 1) is not None), what
        assert all(a[1] == b[0] for a, b in zip(plan, plan[1:])) and plan[0][0] == 0 and plan[-1][1] == case.n_reads, what
        assert sum(sum(c[2]) for c in plan) == case.n_rec, what
        for n_ctx in CONTEXTS:
            mj = model_jobs(plan, n_ctx, case.read_len, case.p)
            assert jobs[n_ctx] == mj, (what, n_ctx, jobs[n_ctx], mj)
            if n_ctx > 1:
                assert jobs[n_ctx] == (case.jobs8 if d4 else case.jobs)[n_ctx], (what, n_ctx)


@pytest.mark.parametrize("case", ROUTED, ids=case_id)
def test_the_routed_bounds_are_the_claimed_ones(case):
    symmetric = case.oracle()["symmetric"] if case.mode < 0 else case.mode
    for n_ctx in CONTEXTS:
        assert model_routed(case.n_reads, case.recs, symmetric, case.n_chunks, n_ctx) == case.bounds[n_ctx], (case, n_ctx)


@pytest.mark.parametrize("case", CASES + ROUTED, ids=case_id)
def test_every_case_fills_the_classes_it_claims(case):
    m = CaseModel(case) if case in CASES else None
    unknown = case.classes - set(CLASSES)
    assert not unknown, unknown
    missed = [cls for cls in case.classes if not holds(cls, case, m)]
    assert not missed, (case, missed)


def test_census_no_class_is_empty():
    models = {c.name: CaseModel(c) for c in CASES}
    empty = [cls for cls in CLASSES if not any(cls in c.classes and holds(cls, c, models.get(c.name)) for c in CASES + ROUTED)]
    assert not empty, empty
