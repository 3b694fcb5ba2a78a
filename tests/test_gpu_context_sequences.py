"""GPU: one engine context over long, seeded call sequences (tests/context_model.py), every pass against the oracle.

A context builds a pass on what its previous one found: speculation without the host wait, the per-read geometry it keeps, the
detecting context's guess, list capacities.  Between passes a caller may change anything the shape key does not cover -- tuning,
output width, cut points, parameters that leave minbins alone, the target columns, other entry points on the same context, the
contents of the same buffers.  After every pass the result, read through a route drawn at random, must equal the oracle's over the
inputs as they are at that moment.  A failing step prints its seed and the op list up to it (replay: ``-k "seed_<n>"``).

The last test checks the paths the library reports (summary flags) were all reached: the long way, speculation with and without the
kept geometry, re-runs and deep tiles."""
import os

import numpy as np
import pytest
from context_model import GROUPED_OPS, N_STEPS, SEEDS, SETS, describe, generate, make_set, params_of
from raft_testlib import ARRAY_KEYS, SCALAR_KEYS, assert_same_result, oracle_run

pytestmark = pytest.mark.gpu

MIN_PER_PATH = 5

_sets: dict = {}
_wants: dict = {}
_flags: dict = {}          # seed -> the summary flags of every pass that went through finish()


def _set(name):
    if name not in _sets:
        _sets[name] = make_set(name)
    return _sets[name]


def _want(name, variant):
    key = (name, variant)
    if key not in _wants:
        c = _set(name)
        mode = SETS[name][1]
        w = oracle_run(params_of(variant, mode), *(c[k] for k in ("read_len", "qid", "qs", "qe", "tid", "ts", "te")))
        if mode == 1:
            w["symmetric"] = 1     # (the target columns repeat the query ones: the oracle piles the query sides only)
        elif mode == 0:
            assert w["symmetric"] == 0, name
        _wants[key] = w
    return _wants[key]


def _scalars(s):
    return dict(symmetric=s.symmetric, high_cov=s.high_cov, total_coverage=s.total_coverage, total_windows=s.total_windows,
                total_repeat_length=s.total_repeat_length, total_read_length=s.total_read_length)


def _check_packed(got, want, what, cov):
    """The arrays a packed route returns (no cut points) against the oracle's, cov already decoded."""
    assert np.array_equal(cov, want["cov"]), f"{what}: cov differs"
    for k in ("cov_offset", "rep_offset", "rep_s", "rep_e", "frag_offset", "frag_begin", "frag_end"):
        assert np.array_equal(np.asarray(got[k]), want[k]), f"{what}: {k} differs"


def _read_back(eng, s, route, width, want, what, rng):
    """The finished pass through one output route, compared with the oracle."""
    import torch
    from raft_amd import hostio
    if route == "fetch":
        got = eng.fetch(); got.update(_scalars(s))
        assert_same_result(got, want, what)
    elif route == "outputs_device":
        o = eng.outputs_device()
        torch.cuda.synchronize()
        got = {k: o[k].cpu().numpy() for k in ARRAY_KEYS}; got.update(_scalars(s))
        assert_same_result(got, want, what)
    elif route == "fetch_packed":
        w = width if width in (1, 2) else rng.choice([1, 2])
        got = eng.fetch_packed(width=w)
        _check_packed(got, want, what, hostio.unpack_coverage(got["cov8"], got["exc_index"], got["exc_value"]))
        assert np.array_equal(got["frag_read"], want["frag_read"]), f"{what}: frag_read differs"
        for k in SCALAR_KEYS:
            assert int(_scalars(s)[k]) == int(want[k]), f"{what}: {k}"
    else:
        got = eng.fetch_delta4()
        _check_packed(got, want, what, hostio.unpack_coverage_d4(s.n_bins, got["cov_nib"], got["cov_anchor"], got["exc_index"], got["exc_value"]))
        for k in SCALAR_KEYS:
            assert int(_scalars(s)[k]) == int(want[k]), f"{what}: {k}"


def run_sequence(seed, n_steps=N_STEPS, ops=None, query=None):
    """Runs generate(seed, n_steps) on one Engine; returns the summary flags of its passes.  Raises with the op list on a mismatch.
    ``ops``: that list with ``{"op": "query", ...}`` entries between its ops (tests/query_sequence_model.py), every one handed to
    ``query(engine, state, flags so far, step, op)`` -- the engine is the second one where the op says ``on="eng2"``."""
    import random

    import torch
    from raft_amd import engine, hostio
    ops = generate(seed, n_steps) if ops is None else ops
    rng = random.Random(seed * 7919 + 1)
    dev = "cuda:0"
    st = {"variant": 0, "mode": None, "width": 4, "tensors": None, "content": None, "finished": False}
    eng = engine.Engine(params_of(0, 1), device=0)
    eng2 = None
    flags = []

    def to_dev(name):
        c = _set(name)
        return {k: torch.from_numpy(c[k]).to(dev) for k in c}

    def ensure_mode(name):
        mode = SETS[name][1]
        if st["mode"] != mode:
            eng.set_params(params_of(st["variant"], mode)); st["mode"] = mode

    try:
        for i, e in enumerate(ops):
            what = f"seed {seed}, step {i} ({e['op']})"
            op = e["op"]
            try:
                if op == "query":
                    query(eng2 if e.get("on") == "eng2" else eng, st, flags, i, e)
                    continue
                if op in ("same", "copy", "alias", "new", "targets"):
                    if op == "same" and st["tensors"] is None:
                        op = "new"; e = dict(e, set=st["content"] or "runs_a")
                    if op == "new":
                        # free, then allocate: the engine's references to the last call's tensors go too, so that the caching
                        # allocator may hand the same addresses out again (the context then sees the old shape key over new tensors)
                        eng._keep = None; eng._last_device_call = None
                        st["tensors"] = None
                        st["tensors"] = to_dev(e["set"]); st["content"] = e["set"]
                    elif op == "copy":
                        src = _set(e["set"])
                        for k, t in st["tensors"].items():
                            t.copy_(torch.from_numpy(src[k]))
                        st["content"] = e["set"]
                    elif op == "alias":                            # new tensor objects over the same memory, other contents
                        src = _set(e["set"])
                        st["tensors"] = {k: t.view(t.shape) for k, t in st["tensors"].items()}
                        for k, t in st["tensors"].items():
                            t.copy_(torch.from_numpy(src[k]))
                        st["content"] = e["set"]
                    elif op == "targets":
                        src = _set(e["set"])
                        for k in ("tid", "ts", "te"):
                            st["tensors"][k] = torch.from_numpy(src[k]).to(dev)
                        for k in ("read_len", "qid", "qs", "qe"):             # (the query side is the same in both mirror states)
                            assert np.array_equal(st["tensors"][k].cpu().numpy(), src[k])
                        st["content"] = e["set"]
                    name = st["content"]
                    ensure_mode(name)
                    t = st["tensors"]
                    eng.run_device(t["read_len"], t["qid"], t["qs"], t["qe"], t["tid"], t["ts"], t["te"])
                    s = eng.finish(); flags.append(s.flags); st["finished"] = True
                    _read_back(eng, s, e["route"], st["width"], _want(name, st["variant"]), what, rng)
                elif op in ("host",) + GROUPED_OPS:
                    name = e["set"]
                    ensure_mode(name)
                    c = _set(name)
                    if op == "host":
                        eng.run_host(c["read_len"], c["qid"], c["qs"], c["qe"], c["tid"], c["ts"], c["te"])
                    else:
                        off = hostio.group_offsets(c["read_len"].size, c["qid"])
                        assert off is not None, name
                        if op == "host_grouped":
                            eng.run_host_grouped(c["read_len"], off, c["qs"], c["qe"])
                        else:
                            win = hostio.pack_windows(c["qs"], c["qe"], params_of(st["variant"], 1).reso)
                            assert win is not None, name
                            eng.run_device_windows(torch.from_numpy(c["read_len"]).to(dev), torch.from_numpy(off).to(dev),
                                                   torch.from_numpy(win.view(np.int32)).to(dev))
                    s = eng.finish(); flags.append(s.flags); st["finished"] = True
                    _read_back(eng, s, e["route"], st["width"], _want(name, st["variant"]), what, rng)
                elif op in ("pipelined1", "pipelined2"):
                    name = e["set"]
                    ensure_mode(name)
                    c = _set(name)
                    st["finished"] = False
                    others = None
                    if op == "pipelined2":
                        if eng2 is None:
                            eng2 = engine.Engine(params_of(st["variant"], st["mode"]), device=0)
                        eng2.set_params(params_of(st["variant"], st["mode"]))
                        others = [eng2]
                    out = eng.host_output_buffers(c["read_len"], pinned=False, width=e["cov_width"])
                    res, s = eng.run_pipelined(c["read_len"], c["qid"], c["qs"], c["qe"], c["tid"], c["ts"], c["te"], n_chunks=e["chunks"],
                                               out=out, others=others)
                    want = _want(name, st["variant"])
                    cov = (hostio.unpack_coverage_d4(s.n_bins, res["cov_nib"], res["cov_anchor"], res["exc_index"], res["exc_value"])
                           if "cov_nib" in res else hostio.unpack_coverage(res["cov8"], res["exc_index"], res["exc_value"]))
                    _check_packed(res, want, what, cov)
                    assert s.total_coverage == want["total_coverage"] and s.total_windows == want["total_windows"], what
                elif op in ("params_keep", "params_minbins"):
                    st["variant"] = e["variant"]
                    st["mode"] = 1 if st["mode"] is None else st["mode"]
                    eng.set_params(params_of(st["variant"], st["mode"]))
                elif op == "width":
                    eng.set_output_width(e["width"]); st["width"] = e["width"]
                elif op == "cuts":
                    eng.set_emit_cuts(e["on"])
                elif op == "tuning":
                    eng.set_tuning(e["tile_bins"], e["force_bucket"])
                elif op == "outputs_edit":
                    # a caller writes into the offsets outputs_device handed out -- in bounds: monotone, ends unchanged, one
                    # interior offset moved by one window -- and then runs the same buffers again
                    # (only right after a pass of this context: a pipelined job's summary does not describe its buffers)
                    if st["tensors"] is None or not st["finished"] or eng.summary.n_reads < 3:
                        continue
                    o = eng.outputs_device()
                    co = o["cov_offset"]
                    h = co.cpu().numpy()
                    ok = np.flatnonzero((h[2:-1] - h[1:-2] >= 2))
                    if ok.size:
                        j = int(ok[rng.randrange(ok.size)]) + 1
                        co[j] += 1
                        torch.cuda.synchronize()
                    t = st["tensors"]
                    ensure_mode(st["content"])
                    eng.run_device(t["read_len"], t["qid"], t["qs"], t["qe"], t["tid"], t["ts"], t["te"])
                    s = eng.finish(); flags.append(s.flags)
                    assert not (s.flags & engine.SUM_KEPT_GEOMETRY), what
                    _read_back(eng, s, e["route"], st["width"], _want(st["content"], st["variant"]), what, rng)
            except Exception as ex:
                raise AssertionError(f"{what}: {ex}\nreplay: -k 'seed_{seed}'; ops so far:\n{describe(ops[:i + 1])}") from ex
    finally:
        eng.close()
        if eng2 is not None:
            eng2.close()
    return flags


@pytest.mark.parametrize("seed", SEEDS, ids=[f"seed_{s}" for s in SEEDS])
def test_context_sequence(seed):
    _flags[seed] = run_sequence(seed)


def test_every_path_was_reached():
    """The paths the library reports over all seeds (missing seeds are run here: -k on one seed leaves this test whole)."""
    from raft_amd import engine
    for seed in SEEDS:
        if seed not in _flags:
            _flags[seed] = run_sequence(seed)
    allf = [f for s in SEEDS for f in _flags[s]]
    S, K = engine.SUM_SPECULATED, engine.SUM_KEPT_GEOMETRY
    counts = {"passes": len(allf),
              "long_way": sum(1 for f in allf if not f & S),
              "speculated_scanned": sum(1 for f in allf if f & S and not f & K),
              "speculated_kept_geometry": sum(1 for f in allf if f & S and f & K),
              "rerun": sum(1 for f in allf if f & engine.SUM_RERUN),
              "deep_tiles": sum(1 for f in allf if f & engine.SUM_DEEP_TILES)}
    print(f"\ncontext sequences, {len(SEEDS)} seeds x {N_STEPS} steps: " + ", ".join(f"{k} {v}" for k, v in counts.items()))
    # (a KEPT_GEOMETRY pass is always a speculated one)
    assert not any(f & K and not f & S for f in allf)
    need = ["long_way", "deep_tiles"]
    if not os.environ.get("RAFT_NO_SPECULATE"):
        need += ["speculated_scanned", "rerun"]
        if not os.environ.get("RAFT_NO_KEEP_GEOMETRY"):
            need += ["speculated_kept_geometry"]
    missing = {k: counts[k] for k in need if counts[k] < MIN_PER_PATH}
    assert not missing, f"paths reached fewer than {MIN_PER_PATH} times: {missing} (all: {counts})"
