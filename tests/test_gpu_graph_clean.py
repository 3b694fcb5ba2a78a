"""GPU: raft_hip_graph_clean_device / _host (raft_amd/csrc/graph_clean.hpp, graph_clean_lib.hip) -- the edge and read states, the rounds,
the degrees, the unitig table, the summary and the error paths -- every output compared in full with the plain-Python rule of
tests/cln_testlib.py; in the device form and the host form, over the sizes at which the kernels stride, long rows, layouts whose answer
is known, the boundary of the weak predicate, and the orders and orientations of one list."""
import os
import re

import numpy as np
import pytest
from cln_testlib import ARRAYS, MUTUAL5, SKIPPED, SUMMARY, TIP, WEAK_U, WEAK_W, Layout, clean
from raft_testlib import ROOT

from raft_amd.params import RaftParams

pytestmark = pytest.mark.gpu

FORMS = ("device", "host")


def constant(header, name):
    text = open(os.path.join(ROOT, "raft_amd", "csrc", header)).read()
    return int(re.search(r"\b%s = (\d+)\b" % name, text).group(1))


THREADS, MAX_BLOCKS = constant("graph_clean.hpp", "kClnThreads"), constant("graph_clean.hpp", "kClnMaxBlocks")
UTG_THREADS, UTG_MAX_BLOCKS = constant("unitig.hpp", "kUtgThreads"), constant("unitig.hpp", "kUtgMaxBlocks")
STRIDE = THREADS * MAX_BLOCKS                      # one full grid-stride of the largest grid, in edges
RANK_STRIDE = UTG_THREADS * UTG_MAX_BLOCKS // 2    # reads beyond which the ranking strides over its half-edges


@pytest.fixture(scope="module")
def eng():
    from raft_amd import engine
    e = engine.Engine(RaftParams(est_cov=3), device=0)
    yield e
    e.close()


def given_arrays(form, arrays, skip):
    import torch
    if form == "host":
        return list(arrays), skip
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    return [dev(a) for a in arrays], None if skip is None else dev(skip)


def compare(got, want, tag):
    assert sorted(got) == sorted(ARRAYS + ("summary", "kernel_seconds", "launches")), tag
    for k in ARRAYS:
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (tag, k, g.dtype, w.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g.ravel() != w.ravel())
        assert bad.size == 0, f"{tag}: {k} differs at {bad.size} places, first at {bad[0]}: got {g.ravel()[bad[0]]} want {w.ravel()[bad[0]]}"
    assert list(got["summary"]) == SUMMARY and got["summary"] == want["summary"], (tag, got["summary"], want["summary"])
    assert got["kernel_seconds"] >= 0.0 and got["launches"] >= 0, tag


def check(eng, arrays, skip=None, W=500, T=3, R=3, what="", forms=FORMS, want=None):
    """Runs the call in every form and compares everything with the oracle (computed once) -> (the wanted dict, the last result)"""
    want = clean(*arrays, skip=skip, W=W, T=T, R=R) if want is None else want
    assert want["error_index"] == -1, (what, want["error_index"])
    got = None
    for form in forms:
        tag = f"{what} ({form}, W={W}, T={T}, R={R}, n_edges={arrays[1].size}, n_reads={arrays[0].size})"
        given, sk = given_arrays(form, arrays, skip)
        got = eng.graph_clean(*given, skip=sk, min_ratio_permille=W, max_tip_reads=T, rounds=R)
        compare(got, want, tag)
        assert got["launches"] > 0 or arrays[0].size == 0, tag
    return want, got


def alive(want, weak=1, tips=1, kept=1, candidates=0):
    """A case cannot pass on a graph where nothing happens: the oracle alone says that it does."""
    s = want["summary"]
    assert s["weak_edges"] >= weak and s["tips"] >= tips and s["kept_edges"] >= kept and s["candidates_kept"] >= candidates, s


def random_graph(rng, n_reads, n_edges):
    """A layout-like graph of exactly that size: a backbone with breaks, extra edges that skip one to four reads, reads turned at
    random, spans at random (so that some edges are weak), the list in a random order and either orientation."""
    L = rng.integers(2000, 5000, n_reads).astype(np.int32)
    if n_edges == 0:
        return L, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32)
    assert n_reads >= 2
    i = np.arange(n_reads - 1, dtype=np.int64)
    back = i[rng.random(i.size) >= 0.05]
    a, b = back, back + 1
    if a.size < n_edges:
        xa = rng.integers(0, n_reads, 3 * (n_edges - a.size) + 8)
        xb = xa + rng.integers(2, 6, xa.size)
        ok = xb < n_reads
        code = np.unique(xa[ok] * n_reads + xb[ok])
        code = code[rng.permutation(code.size)][:n_edges - a.size]
        a, b = np.concatenate([a, code // n_reads]), np.concatenate([b, code % n_reads])
    assert a.size >= n_edges, (n_reads, n_edges, a.size)
    a, b = a[:n_edges], b[:n_edges]
    turned = rng.integers(0, 2, n_reads)
    u, w = 2 * a + (1 - turned[a]), 2 * b + turned[b]
    flip, order = rng.random(n_edges) < 0.5, rng.permutation(n_edges)
    u, w = np.where(flip, w, u)[order], np.where(flip, u, w)[order]
    span = rng.integers(100, 2001, n_edges)
    return L, u.astype(np.int32), w.astype(np.int32), span.astype(np.int32)


def test_the_header_s_constants():
    from raft_amd import engine
    assert (engine.CLN_WEAK_U, engine.CLN_WEAK_W, engine.CLN_TIP) == (WEAK_U, WEAK_W, TIP) == (1, 2, 4)
    assert (engine.CLN_READ_STAYS, engine.CLN_READ_TIP, engine.CLN_READ_FLAGGED) == (0, 1, 2)
    assert (engine.BEST_SKIPPED, engine.BEST_MUTUAL5) == (SKIPPED, MUTUAL5)
    assert (THREADS, MAX_BLOCKS, UTG_THREADS, UTG_MAX_BLOCKS) == (256, 2048, 256, 2048)


# ---- sizes
@pytest.mark.parametrize("n_edges", sorted({0, 1, 2, 63, 64, 65, 255, 256, 257, THREADS - 1, THREADS, THREADS + 1, 2 * THREADS + 1}))
def test_every_number_of_edges(eng, n_edges):
    rng = np.random.default_rng(n_edges + 11)
    arrays = random_graph(rng, max(2, n_edges * 3 // 4 + 2), n_edges)
    want, _ = check(eng, arrays, what="sizes")
    if n_edges >= 63:
        alive(want)
    check(eng, arrays, W=0, T=1, R=1, what="sizes", forms=("device",))


@pytest.mark.parametrize("n_reads", [0, 1, 2, 63, 64, 65])
def test_every_number_of_reads(eng, n_reads):
    rng = np.random.default_rng(n_reads + 3)
    arrays = random_graph(rng, n_reads, 0 if n_reads < 2 else (1 if n_reads == 2 else n_reads + n_reads // 3))
    want, _ = check(eng, arrays, what="reads")
    if n_reads >= 63:
        alive(want)
    if n_reads >= 1:                                                       # (reads that no edge names, some of them flagged)
        skip = np.zeros(n_reads + 5, np.uint8)
        skip[n_reads:n_reads + 3] = (1, 0, 200)
        L = np.concatenate([arrays[0], np.full(5, 300, np.int32)])
        want, _ = check(eng, (L,) + arrays[1:], skip=skip, what="reads and flagged ones")
        assert want["summary"]["reads_flagged"] == 2 and list(want["read_state"][n_reads:]) == [2, 0, 2, 0, 0]
        assert all(want["flags"][n_reads:] == [SKIPPED, 0, SKIPPED, 0, 0])


def test_beyond_one_grid_stride_of_edges_and_of_the_ranking(eng):
    """One list with more edges than the largest grid covers in one stride and more reads than the ranking's grid does: every
    grid-stride loop goes round.  (Once, on the device form: the oracle takes seconds at this size.)"""
    rng = np.random.default_rng(7)
    block_reads, block_edges = 513, 1025
    copies = max(RANK_STRIDE // block_reads, STRIDE // block_edges) + 1
    n_reads, n_edges = copies * block_reads, copies * block_edges
    assert RANK_STRIDE < n_reads and STRIDE < n_edges < STRIDE + 2 * block_edges
    # The list is `copies` disjoint copies of one block, its edges in one random order: the rule looks at nothing beyond a
    # component and shifting the ids keeps their order, so the answer is the block's answer, copy by copy.
    L, u, w, s = random_graph(rng, block_reads, block_edges)
    one = clean(L, u, w, s, T=2, R=2)
    alive(one)
    shift = np.arange(copies, dtype=np.int64)[:, None] * block_reads
    order = rng.permutation(n_edges)
    tiled = lambda a: np.tile(a, (copies,) + (1,) * a.ndim)
    per_edge = lambda a, add=0: (tiled(a) + add).reshape(-1)[order].astype(a.dtype)
    arrays = (tiled(L).reshape(-1), per_edge(u, 2 * shift), per_edge(w, 2 * shift), per_edge(s))
    want = {k: tiled(one[k]).reshape((-1,) + one[k].shape[1:]) for k in ARRAYS}
    want["edge_state"], want["edge_round"] = per_edge(one["edge_state"]), per_edge(one["edge_round"])
    partner = tiled(one["partner"]).astype(np.int64)
    want["partner"] = np.where(partner >= 0, partner + shift[:, :, None], -1).reshape(-1, 2).astype(np.int32)
    same = ("rounds_run", "converged", "longest_row")
    want["summary"] = {k: v if k in same else v * copies for k, v in one["summary"].items()}
    want["error_index"] = -1
    want, got = check(eng, arrays, T=2, R=2, what="strides", forms=("device",), want=want)
    # the table goes into unitigs as it is
    utg = eng.unitigs(arrays[0], got["partner"], got["span"], got["flags"])
    assert utg["summary"]["reads_skipped"] == want["summary"]["tip_reads"]


# ---- rows
@pytest.mark.parametrize("spurs", [1, 2, 63, 64, 65, 300])
def test_a_hub_with_that_many_one_read_spurs(eng, spurs):
    """Read 0's 3' end holds `spurs` arcs to one-read spurs of different lengths: all but the greatest fall, the greatest stays."""
    g = Layout()
    hub = g.read(4000)
    tips = [g.read(1000 + 3 * k) for k in range(spurs)]
    rng = np.random.default_rng(spurs)
    for t in rng.permutation(tips):
        g.join(hub, int(t))
    want, _ = check(eng, g.arrays(), T=1, R=3, what="hub")
    s = want["summary"]
    assert s["longest_row"] == spurs and s["tips"] == spurs - 1 and s["kept_edges"] == 1 and s["converged"] == 1
    assert want["read_state"][tips[-1]] == 0 and all(want["read_state"][tips[:-1]] == 1) and want["read_state"][hub] == 0
    assert s["rounds_run"] == (2 if spurs > 1 else 1) and s["ends_mutual"] == 2 and s["isolated_short"] == 0      # (two reads, T = 1)
    # a hub whose arcs differ in span: the weak cut walks the long row
    g2 = Layout()
    hub = g2.read(4000)
    for k in range(spurs):
        g2.edge(2 * hub + 1, 2 * g2.read(3000), 1000 + k)
    want, _ = check(eng, g2.arrays(), W=999, T=0, R=1, what="hub, weak", forms=("device",))
    assert want["summary"]["weak_edges"] == sum(1 for k in range(spurs) if (1000 + k) * 1000 < 999 * (1000 + spurs - 1))


# ---- known layouts (T = 3)
def main_chain(g, count=40):
    return g.chain(g.reads(count))


def test_spurs_of_one_three_and_four_reads_on_a_chain_of_forty(eng):
    g = Layout()
    main = main_chain(g)
    one, three, four = g.chain(g.reads(1)), g.chain(g.reads(3)), g.chain(g.reads(4))
    for spur in (one, three, four):
        g.join(main[20], spur[0])
    want, _ = check(eng, g.arrays(), what="three spurs")
    s = want["summary"]
    assert (s["tips"], s["tip_reads"], s["rounds_run"], s["converged"], s["weak_edges"]) == (2, 4, 2, 1, 0)
    assert all(want["read_round"][one + three] == 1) and all(want["read_state"][four] == 0) and all(want["read_state"][main] == 0)
    assert s["tip_bases"] == 1000 + (3 * 1000 - 2 * 500) and s["tip_edges"] == 4 and s["kept_edges"] == 39 + 3 + 1


def test_a_spur_at_read_two_falls_and_the_three_read_head_stays(eng):
    g = Layout()
    main = main_chain(g)
    spur = g.read()
    g.join(main[2], spur)
    want, _ = check(eng, g.arrays(), what="head")
    alive(want, weak=0, candidates=0)
    assert want["read_state"][spur] == 1 and all(want["read_state"][main] == 0) and want["summary"]["tips"] == 1
    # the head was a candidate in round 1 and was kept there; in round 2 it is part of the whole chain
    want1, _ = check(eng, g.arrays(), R=1, what="head, one round", forms=("device",))
    assert want1["summary"]["candidates_kept"] == 1 and want1["summary"]["converged"] == 0


@pytest.mark.parametrize("lengths, falls", [((900, 1000), 0), ((1000, 900), 1), ((1000, 1000), 1)])
def test_a_fork_of_two_spurs_at_the_last_end(eng, lengths, falls):
    """Exactly one falls: the shorter one; with equal lengths the larger id."""
    g = Layout()
    main = main_chain(g, 10)
    spurs = [g.read(lengths[0]), g.read(lengths[1])]
    for t in spurs:
        g.join(main[-1], t)
    want, _ = check(eng, g.arrays(), what="fork")
    alive(want, weak=0)
    assert want["read_state"][spurs[falls]] == 1 and want["read_state"][spurs[1 - falls]] == 0 and want["summary"]["tips"] == 1
    want1, _ = check(eng, g.arrays(), R=1, what="fork, one round", forms=("device",))
    alive(want1, weak=0, candidates=1)                                     # (the greater spur was judged and kept)


@pytest.mark.parametrize("R, fallen, rounds_run, converged", [(1, [42], 1, 0), (2, [40, 41, 42, 44], 2, 0), (3, [40, 41, 42, 44], 3, 1)])
def test_a_spur_on_a_spur(eng, R, fallen, rounds_run, converged):
    g = Layout()
    main = main_chain(g)
    g.reads(5)                                                             # 40 .. 44; 43 stands alone
    g.len[42] = 900
    g.join(main[20], 40); g.join(40, 41); g.join(41, 42); g.join(41, 44)
    want, _ = check(eng, g.arrays(), R=R, what="spur on a spur")
    s = want["summary"]
    assert sorted(np.flatnonzero(want["read_state"] == 1)) == fallen and (s["rounds_run"], s["converged"]) == (rounds_run, converged)
    assert want["read_round"][42] == 1 and (R == 1 or list(want["read_round"][[40, 41, 44]]) == [2, 2, 2])
    assert s["isolated_short"] == 1                                        # (read 43)


def test_a_bubble_of_two_branches_loses_nothing(eng):
    g = Layout()
    left, right = main_chain(g, 10), main_chain(g, 10)
    for branch in (g.chain(g.reads(2)), g.chain(g.reads(2))):
        g.join(left[-1], branch[0]); g.join(branch[-1], right[0])
    want, _ = check(eng, g.arrays(), what="bubble")
    s = want["summary"]
    assert (s["tips"], s["weak_edges"], s["converged"], s["rounds_run"], s["kept_edges"]) == (0, 0, 1, 1, len(g.u)) and s["ends_kept_more"] == 2


def test_a_circle_with_a_spur_is_a_circular_unitig_afterwards(eng):
    g = Layout()
    circle = g.reads(12)
    g.chain(circle + [circle[0]])
    spur = g.read()
    g.join(circle[5], spur)
    want, got = check(eng, g.arrays(), what="circle")
    assert want["read_state"][spur] == 1 and want["summary"]["tips"] == 1 and want["summary"]["ends_mutual"] == 24
    utg = eng.unitigs(g.arrays()[0], got["partner"], got["span"], got["flags"])
    assert (utg["summary"]["unitigs"], utg["summary"]["circular"], utg["summary"]["reads_skipped"], utg["summary"]["longest_reads"]) == (1, 1, 1, 12)


@pytest.mark.parametrize("flip", [False, True])
def test_an_edge_that_is_weak_at_one_end_only_falls(eng, flip):
    """End 2 * 0 + 1 holds spans 1000 and 400; the 400 is the best its other end has: weak on one side, and it falls."""
    g = Layout(3000)
    a, x, y = g.reads(3)
    g.join(a, x, 1000)
    e = g.join(a, y, 400)
    arrays = g.arrays(flip=[False, flip])
    want, _ = check(eng, arrays, T=0, what="weak at one end")
    assert want["edge_state"][e] == (WEAK_W if flip else WEAK_U) and want["edge_round"][e] == 0
    assert (want["summary"]["weak_arcs"], want["summary"]["weak_edges"], want["summary"]["kept_edges"]) == (1, 1, 1)
    assert list(want["weak"].ravel()[[2 * a + 1, 2 * y]]) == [1, 1] and list(want["kept"].ravel()[[2 * a + 1, 2 * y]]) == [1, 0]


@pytest.mark.parametrize("W, span, weak", [(500, 1000, False), (500, 999, True), (0, 1, False), (1000, 2000, False), (1000, 1999, True), (1, 1, True)])
def test_the_weak_predicate_at_its_boundary(eng, W, span, weak):
    """span * 1000 == W * m stays, one span unit below it falls (m = 2000; the last case: m = 1001)."""
    g = Layout(3000)
    a, x, y = g.reads(3)
    g.join(a, x, 1001 if W == 1 else 2000)
    e = g.join(a, y, span)
    want, _ = check(eng, g.arrays(), W=W, T=0, R=1, what="weak boundary")
    assert (want["edge_state"][e] != 0) == weak


# ---- orders
def test_the_result_depends_on_no_order_and_no_orientation(eng):
    rng = np.random.default_rng(99)
    L, u, w, s = random_graph(rng, 200, 260)
    want, _ = check(eng, (L, u, w, s), what="as given")
    alive(want)
    for trial in range(3):
        order, flip = rng.permutation(u.size), rng.random(u.size) < 0.5
        u2, w2 = np.where(flip, w, u)[order].astype(np.int32), np.where(flip, u, w)[order].astype(np.int32)
        _, got = check(eng, (L, u2, w2, s[order]), what=f"order {trial}", forms=("device",))
        assert np.array_equal(got["read_state"], want["read_state"]) and np.array_equal(got["partner"], want["partner"])
        assert np.array_equal(got["edge_round"], want["edge_round"][order])
        assert np.array_equal(got["edge_state"] != 0, (want["edge_state"] != 0)[order]) and got["summary"] == want["summary"]


def test_behind_string_graph_and_in_front_of_unitigs(eng):
    """string_graph -> graph_clean -> unitigs composes without a conversion."""
    from sg_testlib import contained, layout
    L, cols, strand, _ = layout(np.random.default_rng(5), 60)
    skip = contained(L, cols, strand)
    res = eng.string_graph(L, *cols, strand, skip=skip)
    assert res["n_out"] > 0
    arrays = (L, res["edge_u"], res["edge_w"], res["edge_span"])
    want, c = check(eng, arrays, skip=skip, T=4, what="behind string_graph", forms=("host",))
    assert np.array_equal(c["arcs"], res["kept"])
    utg = eng.unitigs(L, c["partner"], c["span"], c["flags"])
    assert utg["summary"]["reads_skipped"] == want["summary"]["reads_flagged"] + want["summary"]["tip_reads"]


# ---- errors
def bad_lists():
    g = Layout(1000)
    g.chain(g.reads(6))
    L, u, w, s = g.arrays()
    skip = np.zeros(6, np.uint8)
    skip[5] = 1                                                            # (edge 4 names read 5)
    yield "a flagged read", (L, u, w, s), skip, 4
    for what, col, at, value in (("u below 0", 1, 3, -1), ("u beyond the nodes", 1, 2, 12), ("w beyond the nodes", 2, 1, 1 << 30), ("w below 0", 2, 4, -7),
                                 ("one read twice", 2, 2, 4), ("span 0", 3, 3, 0), ("span beyond the shorter read", 3, 0, 1001)):
        cols = [L, u.copy(), w.copy(), s.copy()]
        cols[col][at] = value
        yield what, tuple(cols), None, at
    yield "a pair twice", (L, np.append(u, u[1]), np.append(w, w[1]), np.append(s, 77).astype(np.int32)), None, 5
    yield "a pair twice, turned", (L, np.append(u, w[3]), np.append(w, u[3]), np.append(s, 500).astype(np.int32)), None, 5
    yield "two bad edges", (L, np.array([1, 3, 99, 1], np.int32), np.array([2, 4, 0, 2], np.int32), np.full(4, 500, np.int32)), None, 2
    Ls = L.copy()
    Ls[2] = -5                                                             # (a negative length counts as 0: no span fits)
    yield "a negative length", (Ls, u, w, s), None, 1


@pytest.mark.parametrize("what, arrays, skip, index", list(bad_lists()), ids=[b[0] for b in bad_lists()])
def test_a_bad_edge_is_reported_with_the_smallest_index(eng, what, arrays, skip, index):
    from raft_amd import engine
    assert clean(*arrays, skip=skip)["error_index"] == index, what
    for form in FORMS:
        given, sk = given_arrays(form, arrays, skip)
        with pytest.raises(engine.RaftError) as err:
            eng.graph_clean(*given, skip=sk)
        assert err.value.code == engine.ERR_READ_ID and err.value.index == index and "graph_clean:" in str(err.value), (what, form)


def test_no_read_and_an_edge_is_a_bad_edge(eng):
    from raft_amd import engine
    with pytest.raises(engine.RaftError) as err:
        eng.graph_clean(np.zeros(0, np.int32), np.array([0], np.int32), np.array([2], np.int32), np.array([5], np.int32))
    assert err.value.code == engine.ERR_READ_ID and err.value.index == 0


@pytest.mark.parametrize("kw", [dict(min_ratio_permille=-1), dict(min_ratio_permille=1001), dict(max_tip_reads=-1), dict(rounds=0), dict(rounds=65)])
def test_refusals_name_the_call(eng, kw):
    from raft_amd import engine
    g = Layout()
    g.chain(g.reads(3))
    with pytest.raises(engine.RaftError) as err:
        eng.graph_clean(*g.arrays(), **kw)
    assert err.value.code == engine.ERR_PARAM and "graph_clean:" in str(err.value)
    assert eng.last_graph_clean_launches == 0


def test_what_the_binding_cannot_ask_is_refused_by_the_library(eng):
    """Sizes beyond int32 nodes and arcs, negative counts and missing inputs, through the entry points themselves: refused before any
    launch and before any array is read (the arrays here hold one element)."""
    import ctypes as C

    from raft_amd import _marshal as M
    from raft_amd import engine
    cln = engine.load_side_library("cln")
    one = np.ones(1, np.int32)
    p, null = M.ptr(one), None
    cases = [((2 ** 30, p, 0, null, null, null), engine.ERR_TOO_LARGE), ((1, p, 2 ** 30, p, p, p), engine.ERR_TOO_LARGE),
             ((-1, p, 0, null, null, null), engine.ERR_PARAM), ((1, p, -1, p, p, p), engine.ERR_PARAM), ((1, null, 0, null, null, null), engine.ERR_PARAM),
             ((2, p, 1, null, p, p), engine.ERR_PARAM), ((2, p, 1, p, null, p), engine.ERR_PARAM), ((2, p, 1, p, p, null), engine.ERR_PARAM)]
    for fn in (cln.raft_hip_graph_clean_host, cln.raft_hip_graph_clean_device):
        for (n_reads, L, n_edges, u, w, s), code in cases:
            launches = np.full(1, 77, np.int64)
            rc = fn(eng._ctx, n_reads, L, null, n_edges, u, w, s, 500, 4, 3, *[null] * 10, None, None, None, launches.ctypes.data_as(C.POINTER(C.c_int64)))
            assert rc == code and launches[0] == 77, (n_reads, n_edges, rc)
            with pytest.raises(engine.RaftError, match="graph_clean:"):
                eng._check(rc)
    assert (2 ** 30 - 1, 2 ** 30 - 1) == (engine.UTG_MAX_READS, engine.CTN_MAX_READS)      # (the greatest sizes that are taken are not run here)


def test_the_bounds_of_the_parameters_are_taken(eng):
    g = Layout()
    main = main_chain(g, 8)
    g.join(main[3], g.read())
    for W, T, R in ((0, 0, 1), (1000, 2 ** 31 - 1, 64), (1000, 0, 64)):
        want, got = check(eng, g.arrays(), W=W, T=T, R=R, what="bounds", forms=("host",))
        assert want["summary"]["converged"] == 1 and want["summary"]["rounds_run"] <= 2
    assert eng.last_graph_clean_launches == got["launches"] > 0 and eng.last_graph_clean_seconds == got["kernel_seconds"]
