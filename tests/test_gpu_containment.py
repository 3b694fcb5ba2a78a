"""GPU: raft_hip_containment_device / _host and raft_hip_place_contained_device / _host (raft_amd/csrc/containment.hpp,
containment_lib.hip) -- every output array and every summary field compared exactly with the sequential walk of tests/ctn_testlib.py;
in the device form and the host form, over the sizes at which the streaming kernels change path, the depths at which the round count
changes, the ties of the rule, the orders of one stream, and the error paths."""
import ctypes as C

import numpy as np
import pytest
from ctn_testlib import (HAS_PARENT, ORPHAN, PARENT_REV, PER_READ, PLACE_PER_READ, PLACE_PER_UNITIG, PLACE_SUMMARY, ROOT_REV, SUMMARY, UNPLACED_VIEW,
                         chain, oracle, place_oracle, records, reordered, rounds, star, whole_inside)
from test_gpu_components import given_arrays
from test_gpu_overlap_ends import SIZES, STRIDE, T, make_stream, mirrored

from raft_amd.params import RaftParams

pytestmark = pytest.mark.gpu

FORMS = ("device", "host")
NONE = ([np.zeros(0, np.int32)] * 6, np.zeros(0, np.uint8))


@pytest.fixture(scope="module")
def eng():
    from raft_amd import engine
    e = engine.Engine(RaftParams(est_cov=3), device=0)
    yield e
    e.close()


def compare(got, want, tag, table=PER_READ, summary=SUMMARY):
    assert sorted(got) == sorted(list(table) + ["summary", "kernel_seconds"]), tag
    for k, dt in table.items():
        g, w = got[k], want[k]
        assert g.dtype == dt and g.shape == w.shape, (tag, k, g.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, f"{tag}: {k} differs at {bad.size} places, first at {bad[0]}: got {g[bad[0]]} want {w[bad[0]]}"
    assert list(got["summary"]) == summary and got["summary"] == want["summary"], (tag, got["summary"], want["summary"])
    assert got["kernel_seconds"] >= 0.0, tag


def check(eng, L, cols, strand, H=1000, F=800, symmetric=False, what="", forms=FORMS, offset=False, want=None):
    """Runs the call in every form and compares everything with the oracle (computed once) -> (the wanted dict, the last result)"""
    want = oracle(L, cols, strand, H, F, symmetric) if want is None else want
    got = None
    for form in forms:
        tag = f"{what} ({form}, H={H}, F={F}, symmetric={symmetric}, n_rec={cols[0].size}, n_reads={L.size})"
        got = eng.containment(*given_arrays(form, L, cols, strand, offset), max_overhang=H, min_ratio_permille=F, symmetric=symmetric)
        compare(got, want, tag)
    return want, got


def test_the_header_s_constants():
    from raft_amd import engine
    assert (engine.CTN_HAS_PARENT, engine.CTN_PARENT_REV, engine.CTN_ROOT_REV, engine.CTN_UNPLACED_VIEW, engine.CTN_ORPHAN) == \
        (HAS_PARENT, PARENT_REV, ROOT_REV, UNPLACED_VIEW, ORPHAN) == (1, 2, 4, 8, 16)
    assert [k for k, _ in engine.CTN_PER_READ] == list(PER_READ) and dict(engine.CTN_PER_READ) == PER_READ
    assert (T, STRIDE) == (1024, 2048 * 1024) and [rounds(n) for n in (0, 1, 2, 3, 4, 5, 1024, 1025)] == [1, 1, 1, 2, 2, 3, 10, 11]


# ---- sizes
@pytest.mark.parametrize("n_rec", SIZES)
def test_every_number_of_records(eng, n_rec):
    rng = np.random.default_rng(n_rec + 17)
    L, cols, strand = make_stream(rng, 65 if n_rec < STRIDE else 3000, n_rec)
    want, _ = check(eng, L, cols, strand, what="sizes")
    if n_rec < STRIDE:                           # (the oracle of the largest stream takes seconds: once)
        check(eng, L, cols, strand, symmetric=True, what="sizes", forms=("device",))
    if n_rec >= 2 * T:
        s = want["summary"]
        assert s["reads_with_parent"] > 0 and s["greatest_depth"] > 1 and s["containment_views"] > s["reads_with_parent"]


@pytest.mark.parametrize("n_reads", [0, 1, 2, 255, 256, 257])
def test_every_number_of_reads(eng, n_reads):
    rng = np.random.default_rng(n_reads)
    L, cols, strand = make_stream(rng, n_reads, 4 * n_reads + 3) if n_reads else (np.zeros(0, np.int32), *NONE)
    want, _ = check(eng, L, cols, strand, what="reads")
    if n_reads >= 255:
        assert 0 < want["summary"]["reads_with_parent"] < n_reads
    # ... and without records: every read a root
    want, got = check(eng, L, *NONE, what="no records")
    assert want["summary"]["roots"] == n_reads and np.array_equal(got["root"], np.arange(n_reads)) and not got["flags"].any()
    assert (got["parent"] == -1).all() and not got["children"].any() and want["summary"]["launches"] == (3 + rounds(n_reads) if n_reads else 0)


@pytest.mark.parametrize("n_rec", [1, 5, 257, 2 * T + 3])
def test_columns_off_the_16_byte_line(eng, n_rec):
    rng = np.random.default_rng(n_rec)
    L, cols, strand = make_stream(rng, 65, n_rec)
    check(eng, L, cols, strand, what="misaligned", forms=("device",), offset=True)


# ---- depths: the edges of the round count, the composition at every round
@pytest.mark.parametrize("strands", ["alternating", "random"])
@pytest.mark.parametrize("depth", [1, 2, 3, 4, 5, 31, 32, 33, 1000])
def test_chains(eng, depth, strands):
    bits = np.arange(depth) & 1 if strands == "alternating" else np.random.default_rng(depth).integers(0, 2, depth)
    L, cols, strand = chain(depth, bits)
    want, got = check(eng, L, cols, strand, what=f"chain {depth} {strands}")
    s = want["summary"]
    assert s["greatest_depth"] == depth == s["largest_tree_reads"] and s["roots"] == 1 and s["orphans"] == 0
    assert sorted(got["depth"].tolist()) == list(range(depth + 1)) and got["flags"].max() <= (HAS_PARENT | PARENT_REV | ROOT_REV)
    if depth >= 3:
        assert (got["flags"] & ROOT_REV != 0).any() and ((got["flags"] & ROOT_REV != 0) != (got["flags"] & PARENT_REV != 0)).any()


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("n_children", [65, 257, 5000])
def test_stars(eng, n_children, shuffle):
    L, cols, strand = star(n_children, shuffle=shuffle)
    want, got = check(eng, L, cols, strand, what=f"star {n_children}")
    assert got["children"][0] == n_children == got["tree_reads"][0] and want["summary"]["greatest_depth"] == 1
    assert got["tree_bases"][0] == int(L[1:].astype(np.int64).sum())


# ---- ties
def test_equal_lengths_and_ids(eng):
    L = np.array([5000, 5000, 5000, 7000], np.int32)
    # reads 0, 1, 2 whole against each other: the larger id lies in the smaller; read 2 has two containers of one length: the smaller id
    cols, strand = records([(1, 0, 5000, 0, 0, 5000, 0), (2, 0, 5000, 1, 0, 5000, 1), (0, 0, 5000, 2, 0, 5000, 0), (2, 0, 5000, 3, 100, 5100, 0)])
    want, got = check(eng, L, cols, strand, what="equal lengths")
    assert got["parent"].tolist() == [-1, 0, 3, -1] and not (got["flags"] & UNPLACED_VIEW).any()
    # a read as long as its container, one base of the container left over: in the smaller id it is placed, in the larger it is not
    for r, c, parent in ((1, 0, 0), (0, 1, -1)):
        cols, strand = records([(r, 0, 5000, c, 1, 5000, 0)])
        want, got = check(eng, L, cols, strand, what=f"as long as its container {r} in {c}")
        assert got["parent"][r] == parent and want["summary"]["containment_views"] == 1
        assert got["flags"][r] == (HAS_PARENT if parent >= 0 else UNPLACED_VIEW | ORPHAN) and want["summary"]["orphans"] == (parent < 0)


def test_the_pair_that_would_be_a_cycle(eng):
    L = np.array([1000, 1010, 3000], np.int32)
    # 0 lies in 1; 1, longer by an indel, lies in 0: one parent, one view that places nobody, no cycle; 1 then lies nowhere else ...
    cols, strand = records([(0, 0, 1000, 1, 5, 1005, 0), (1, 0, 1010, 0, 1, 1000, 0)])
    want, got = check(eng, L, cols, strand, what="cycle")
    assert got["parent"].tolist() == [1, -1, -1] and got["flags"].tolist() == [HAS_PARENT, UNPLACED_VIEW | ORPHAN, 0]
    assert (want["summary"]["views_not_longer"], want["summary"]["orphans"], want["summary"]["greatest_depth"]) == (1, 1, 1)
    # ... and once 2 holds it, it is no orphan, keeps its flag, and 0 is two deep
    cols, strand = records([(0, 0, 1000, 1, 5, 1005, 1), (1, 0, 1010, 0, 1, 1000, 0), (2, 200, 1210, 1, 0, 1010, 1)])
    want, got = check(eng, L, cols, strand, what="cycle held")
    assert got["parent"].tolist() == [1, 2, -1] and got["flags"][1] == (HAS_PARENT | PARENT_REV | ROOT_REV | UNPLACED_VIEW) and got["depth"][0] == 2
    assert got["flags"][0] == (HAS_PARENT | PARENT_REV) and want["summary"]["orphans"] == 0


def test_several_records_of_one_pair(eng):
    L = np.array([9000, 5000, 9000], np.int32)
    rows = [(1, 0, 5000, 0, 100, 5100, 0),           # the whole read, '+', at 100
            (1, 0, 5000, 0, 90, 5090, 1),            # the whole read, '-': before '+' at one span
            (1, 0, 5000, 0, 80, 5080, 1),            # ... and the smaller pos wins
            (1, 10, 4990, 0, 50, 5030, 0),           # a shorter span loses whatever its place
            (0, 85, 5085, 1, 0, 5000, 1),            # the target's view of a record written from the container
            (1, 0, 5000, 2, 4000, 9000, 0)]          # a container as long with the larger id: never the parent
    cols, strand = records(rows)
    want, got = check(eng, L, cols, strand, what="one pair")
    assert (got["parent"][1], got["pos"][1], got["span"][1], got["flags"][1]) == (0, 80, 5000, HAS_PARENT | PARENT_REV | ROOT_REV)
    want, got = check(eng, L, *records(rows[:1] + rows[3:4]), what="one pair, two")
    assert (got["pos"][1], got["span"][1], got["flags"][1]) == (100, 5000, HAS_PARENT)
    # the clamp: the query's span longer than the target's by an indel pushes the raw place beyond lc - lr
    L2 = np.array([5000, 5010], np.int32)
    want, got = check(eng, L2, *records([(0, 0, 5000, 1, 15, 5010, 0)]), what="clamp")
    assert (got["parent"][0], got["pos"][0], got["span"][0]) == (1, 10, 4995)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_a_run_of_one_query_across_lanes_and_waves(eng, where):
    n = 3 * 256 + 7                              # three waves' worth of one query id and a tail
    L = np.concatenate([[4000], np.full(n, 9000)]).astype(np.int32)
    L[1 + {"first": 0, "middle": n // 2, "last": n - 1}[where]] = 9001          # the longest container: the parent
    rng = np.random.default_rng(n)
    rows = [whole_inside(0, c, L, int(rng.integers(0, 5000)), int(rng.integers(0, 2))) for c in range(1, n + 1)]
    want, got = check(eng, L, *records(rows), what=f"run, best {where}")
    assert got["parent"][0] == int(np.argmax(L)) and want["summary"]["containment_views"] == n
    # ... and one container named by every record: the best place first, in the middle, last
    L = np.array([4000, 9000], np.int32)
    rows = [whole_inside(0, 1, L, 1000 + k, 0) for k in range(n)]
    best = {"first": 0, "middle": n // 2, "last": n - 1}[where]
    rows[best] = whole_inside(0, 1, L, 7, 0)
    want, got = check(eng, L, *records(rows), what=f"run, best place {where}")
    assert (got["parent"][0], got["pos"][0]) == (1, 7)


# ---- orders
def test_five_permutations_give_equal_bytes(eng):
    rng = np.random.default_rng(5)
    L, cols, strand = make_stream(rng, 300, 4 * T + 3)
    want, first = check(eng, L, cols, strand, what="sorted", forms=("device",))
    for k in range(5):
        order = rng.permutation(cols[0].size)
        pc, ps = reordered(cols, strand, order)
        _, got = check(eng, L, pc, ps, what=f"permutation {k}", forms=("device",) if k else FORMS, want=want)
        assert all(got[key].tobytes() == first[key].tobytes() for key in PER_READ) and got["summary"] == first["summary"]


@pytest.mark.parametrize("H,F", [(1000, 800), (0, 1000)])
def test_a_mirrored_stream_on_its_query_sides_is_its_half_on_both(eng, H, F):
    rng = np.random.default_rng(H + F)
    L, cols, strand = make_stream(rng, 65, 2 * T + 3)
    _, half = check(eng, L, cols, strand, H=H, F=F, what="half", forms=("device",))
    full_cols, full_strand = mirrored(cols, strand)
    _, full = check(eng, L, full_cols, full_strand, H=H, F=F, symmetric=True, what="mirrored")
    assert all(np.array_equal(full[k], half[k]) for k in PER_READ)
    assert all(full["summary"][k] == half["summary"][k] for k in SUMMARY[1:-1])


# ---- errors
def raw_call(eng, form, L, cols, strand, outs, H=1000, F=800, symmetric=0, n_reads=None, n_rec=None, sum_=None):
    """The entry point itself, with the caller's output arrays -> (code, error_index, the context's message)"""
    import torch
    from raft_amd import engine
    lib = engine.load_side_library("ctn")
    arrays = [L] + list(cols) + [strand]
    if form == "device":
        held = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays]
        eng.use_torch_stream()
        fn = lib.raft_hip_containment_device
    else:
        held, fn = arrays, lib.raft_hip_containment_host
    p = [engine.M.ptr(a) for a in held]
    err = C.c_int64(-5)
    rc = fn(eng._ctx, L.size if n_reads is None else n_reads, p[0], cols[0].size if n_rec is None else n_rec, *p[1:], H, F, symmetric,
            *[engine.M.ptr(o) for o in outs], None if sum_ is None else C.byref(sum_), C.byref(err), None)
    return rc, err.value, eng._lib.raft_hip_last_error(eng._ctx).decode()


def marked_outputs(n):
    return [np.full(n, 77, dt) for dt in PER_READ.values()]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("column", [0, 3])
def test_the_first_bad_id_is_reported_and_the_outputs_stay(eng, form, column):
    from raft_amd import engine
    rng = np.random.default_rng(3)
    L, cols, strand = make_stream(rng, 65, 2 * T + 3)
    for at, value in ((2 * T + 1, 65), (T + 5, -1), (700, 1 << 30)):
        cols[column][at] = value                 # (each one in front of the one before)
        outs = marked_outputs(65)
        rc, index, message = raw_call(eng, form, L, cols, strand, outs)
        assert (rc, index) == (engine.ERR_READ_ID, at) and message.startswith("containment:"), (rc, index, message)
        assert all((o == 77).all() for o in outs)
    with pytest.raises(engine.RaftError) as e:
        eng.containment(*given_arrays(form, L, cols, strand))
    assert e.value.code == engine.ERR_READ_ID and e.value.index == 700
    # without reads every id is out of range
    rc, index, _ = raw_call(eng, form, np.zeros(0, np.int32), [c[:3] for c in cols], strand[:3], [None] * 11)
    assert (rc, index) == (engine.ERR_READ_ID, 0)


@pytest.mark.parametrize("form", FORMS)
def test_every_refusal(eng, form):
    from raft_amd import engine
    rng = np.random.default_rng(4)
    L, cols, strand = make_stream(rng, 9, 20)
    outs = marked_outputs(9)
    cases = [(dict(H=-1), engine.ERR_PARAM), (dict(F=-1), engine.ERR_PARAM), (dict(F=1001), engine.ERR_PARAM), (dict(n_reads=-1), engine.ERR_PARAM),
             (dict(n_rec=-1), engine.ERR_PARAM), (dict(n_reads=(1 << 30)), engine.ERR_TOO_LARGE)]
    for kw, code in cases:
        rc, index, message = raw_call(eng, form, L, cols, strand, outs, **kw)
        assert rc == code and index == -5 and message.startswith("containment:"), (kw, rc, message)
    for missing in range(8):
        arrays = [L] + list(cols) + [strand]
        arrays[missing] = None
        rc, index, message = raw_call(eng, form, arrays[0] if arrays[0] is not None else np.zeros(0, np.int32), arrays[1:7], arrays[7], outs,
                                      n_reads=9, n_rec=20)
        assert rc == engine.ERR_PARAM and index == -5 and message.startswith("containment:"), (missing, rc, message)
    assert all((o == 77).all() for o in outs)
    # the context is as good as before
    check(eng, L, cols, strand, what="after the refusals", forms=(form,))


@pytest.mark.parametrize("form", FORMS)
def test_every_output_may_be_null(eng, form):
    from raft_amd import engine
    rng = np.random.default_rng(6)
    L, cols, strand = make_stream(rng, 65, 2 * T + 3)
    want = oracle(L, cols, strand)
    rc, index, _ = raw_call(eng, form, L, cols, strand, [None] * 11)
    assert (rc, index) == (engine.OK, -1)
    for k, key in enumerate(PER_READ):           # one output at a time, and the summary alone
        outs = [None] * 11
        outs[k] = np.full(65, 77, PER_READ[key])
        assert raw_call(eng, form, L, cols, strand, outs)[0] == engine.OK and np.array_equal(outs[k], want[key]), key
    sm = engine._CtnSummary()
    assert raw_call(eng, form, L, cols, strand, [None] * 11, sum_=sm)[0] == engine.OK and engine._summary_dict(sm) == want["summary"]


def test_calls_of_falling_and_rising_size_on_one_context(eng):
    rng = np.random.default_rng(8)
    for n_reads, n_rec in ((3000, 3 * T), (65, 300), (1, 0), (257, T + 1), (0, 0), (3000, 2 * T + 3), (2, 5)):
        L, cols, strand = make_stream(rng, n_reads, n_rec) if n_reads else (np.zeros(0, np.int32), *NONE)
        check(eng, L, cols, strand, what=f"sequence {n_reads} {n_rec}")


# ---- the second call
def layout(eng, L, partner_rows):
    """The layout of raft_hip_unitigs_* for a table of mutual ends: rows of (read, end, partner, partner's end, span)"""
    from raft_amd import engine
    n = L.size
    partner, span, flags = np.full((n, 2), -1, np.int32), np.zeros((n, 2), np.int32), np.zeros(n, np.uint8)
    for r, e, p, pe, s in partner_rows:
        for a, ae, b, be in ((r, e, p, pe), (p, pe, r, e)):
            partner[a, ae], span[a, ae] = b, s
            flags[a] |= (engine.BEST_MUTUAL5 if ae == 0 else engine.BEST_MUTUAL3) | ((engine.BEST_REV5 if ae == 0 else engine.BEST_REV3) if ae == be else 0)
    return partner, span, flags


def place_check(eng, L, forest, utg, what, unitig=None, n_utg=None):
    unitig = utg["unitig"] if unitig is None else unitig
    lengths = utg["utg_length"] if n_utg is None else utg["utg_length"][:n_utg]
    want = place_oracle(L, forest, unitig, utg["offset"], utg["orient"], lengths)
    got = None
    for form in FORMS:
        import torch
        dev = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")) if form == "device" else (lambda a: a)
        f = {k: dev(forest[k]) for k in ("root", "root_pos", "flags")}
        got = eng.place_contained(dev(L), f, dev(unitig), dev(utg["offset"]), dev(utg["orient"]), dev(lengths))
        compare(got, want, f"{what} ({form})", table={**PLACE_PER_READ, **PLACE_PER_UNITIG}, summary=PLACE_SUMMARY)
    return want, got


def backbone_with_trees(eng, ends, circular=False):
    """Six backbone reads 0 .. 5 of 20000 bases joined end to end by `ends` (pairs of the ends that meet), reads 6 .. 11 inside them
    one and two deep on both strands, read 12 alone, read 13 an orphan with read 14 inside it.  -> L, forest, layout, skip"""
    L = np.array([20000] * 6 + [5000, 3000, 6000, 2000, 7000, 1000, 9000, 4000, 2500], np.int32)
    rows = [whole_inside(6, 0, L, 100, 0), whole_inside(7, 6, L, 50, 1), whole_inside(8, 2, L, 14000, 1), whole_inside(9, 8, L, 3999, 1),
            whole_inside(10, 5, L, 0, 0, from_target=True), whole_inside(11, 10, L, 6000, 0),
            (13, 0, 4000, 14, 1, 2500, 0),           # 13 (4000 bases) in 14 (2500): not acceptable, and nothing else holds 13: an orphan
            whole_inside(14, 13, L, 700, 1)]
    cols, strand = records(rows)
    forest = eng.containment(L, *cols, strand, max_overhang=2000, min_ratio_permille=0)
    want = oracle(L, cols, strand, 2000, 0)
    compare(forest, want, "forest")
    assert forest["flags"][13] & ORPHAN and forest["root"][14] == 13 and forest["depth"].max() == 2
    joins = [(a, ea, b, eb, 1000) for (a, ea), (b, eb) in ends]
    partner, span, flags = layout(eng, L, joins)
    skip = (forest["parent"] >= 0) | (forest["flags"] & ORPHAN != 0)
    flags[skip] = 16
    utg = eng.unitigs(L, partner, span, flags)
    assert (utg["unitig"][skip] == -1).all() and bool(utg["utg_circular"].any()) == circular
    return L, forest, utg


def test_placement_on_a_path_walked_forward_and_backward(eng):
    # 0 -> 1 -> ... -> 5, all '+': 3' of k meets 5' of k + 1
    L, forest, utg = backbone_with_trees(eng, [((k, 1), (k + 1, 0)) for k in range(5)])
    want, got = place_check(eng, L, forest, utg, "path +")
    assert not utg["orient"][:6].any() and want["summary"]["unplaced"] == 2 and want["summary"]["unitigs_gained"] == 1
    assert got["placed_unitig"][13] == got["placed_unitig"][14] == -1 and got["start"][7] == 100 + 50
    # the same reads, every second one flipped: the walk enters 1, 3, 5 at their 3' ends
    ends = [((k, 1 if k % 2 == 0 else 0), (k + 1, 1 if k % 2 == 0 else 0)) for k in range(5)]
    L, forest, utg = backbone_with_trees(eng, ends)
    want, got = place_check(eng, L, forest, utg, "path + -")
    assert utg["orient"][:6].tolist() == [0, 1, 0, 1, 0, 1] and got["placed_orient"][10] == 1 and got["start"][10] == utg["offset"][5] + 13000


def test_placement_on_a_cycle_singletons_and_an_orphan_s_tree(eng):
    ends = [((k, 1), ((k + 1) % 6, 0)) for k in range(6)]
    L, forest, utg = backbone_with_trees(eng, ends, circular=True)
    want, got = place_check(eng, L, forest, utg, "cycle")
    assert want["summary"]["n_unitigs"] == 2 and want["summary"]["placed"] == 13          # the cycle and read 12 alone
    # singletons: no joins at all
    L, forest, utg = backbone_with_trees(eng, [])
    want, got = place_check(eng, L, forest, utg, "singletons")
    assert want["summary"]["n_unitigs"] == 7 and want["summary"]["unitigs_gained"] == 3 and got["placed_reads"].tolist() == [3, 1, 3, 1, 1, 3, 1]


@pytest.mark.parametrize("form", FORMS)
def test_placement_refuses_a_table_it_cannot_trust(eng, form):
    from raft_amd import engine
    L, forest, utg = backbone_with_trees(eng, [((k, 1), (k + 1, 0)) for k in range(5)])
    import torch
    dev = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")) if form == "device" else (lambda a: a)

    def call(forest, unitig, lengths):
        f = {k: dev(forest[k]) for k in ("root", "root_pos", "flags")}
        return eng.place_contained(dev(L), f, dev(unitig), dev(utg["offset"]), dev(utg["orient"]), dev(lengths))
    for at, value in ((9, 1), (4, -2), (2, 7)):      # (each one in front of the one before; the layout has one unitig of six and read 12)
        unitig = utg["unitig"].copy()
        unitig[at] = value if value < 0 else utg["utg_length"].size + value - 1
        with pytest.raises(engine.RaftError) as e:
            call(forest, unitig, utg["utg_length"])
        assert e.value.code == engine.ERR_READ_ID and e.value.index == at and "place_contained:" in str(e.value)
    for at, value in ((11, 15), (3, -1)):
        bad = dict(forest, root=forest["root"].copy())
        bad["root"][at] = value
        with pytest.raises(engine.RaftError) as e:
            call(bad, utg["unitig"], utg["utg_length"])
        assert e.value.code == engine.ERR_READ_ID and e.value.index == at
    # n_unitigs 0: every read that names a unitig is out of range; reads that name none are unplaced
    with pytest.raises(engine.RaftError) as e:
        call(forest, utg["unitig"], utg["utg_length"][:0])
    assert e.value.code == engine.ERR_READ_ID and e.value.index == 0
    none = np.full(L.size, -1, np.int32)
    got = call(forest, none, utg["utg_length"][:0])
    want = place_oracle(L, forest, none, utg["offset"], utg["orient"], utg["utg_length"][:0])
    compare(got, want, "no unitigs", table={**PLACE_PER_READ, **PLACE_PER_UNITIG}, summary=PLACE_SUMMARY)
    assert got["summary"]["unplaced"] == L.size
    # no reads
    e0 = np.zeros(0, np.int32)
    got = eng.place_contained(e0, dict(root=e0, root_pos=e0, flags=np.zeros(0, np.uint8)), e0, np.zeros(0, np.int64), np.zeros(0, np.uint8), np.zeros(0, np.int64))
    assert got["summary"] == dict.fromkeys(PLACE_SUMMARY, 0)
    # the refusals of the entry point
    lib = engine.load_side_library("ctn")
    fn = lib.raft_hip_place_contained_host
    p = [engine.M.ptr(a) for a in (L, forest["root"], forest["root_pos"], forest["flags"], utg["unitig"], utg["offset"], utg["orient"])]
    lengths = engine.M.ptr(np.ascontiguousarray(utg["utg_length"]))
    for n, arrays, n_utg, lens, code in ((-1, p, 2, lengths, engine.ERR_PARAM), (15, p, -1, lengths, engine.ERR_PARAM), (15, p, 2, None, engine.ERR_PARAM),
                                         (15, p[:3] + [None] + p[4:], 2, lengths, engine.ERR_PARAM), (1 << 30, p, 2, lengths, engine.ERR_TOO_LARGE)):
        assert fn(eng._ctx, n, *arrays, n_utg, lens, *[None] * 9) == code
        assert eng._lib.raft_hip_last_error(eng._ctx).decode().startswith("place_contained:")
    assert fn(eng._ctx, 15, *p, int(utg["utg_length"].size), lengths, *[None] * 9) == engine.OK          # every output NULL
