"""GPU: raft_hip_components_device / _host (raft_amd/csrc/components.hpp, components_lib.hip) -- the component and the degree of every
read, the row of every component, the summary and the error paths -- every output compared in full with the sequential union-find of
tests/cc_testlib.py; in the device form and the host form, over the sizes at which the kernels change path, the graph shapes that
break a union, the masks, and the orders of one stream."""
import ctypes as C

import numpy as np
import pytest
from cc_testlib import KINDS_ALL, KINDS_PROPER, PER_COMPONENT, PER_READ, SUMMARY, edge_mask, edge_stream, oracle, reordered
from test_gpu_overlap_ends import SIZES, STRIDE, T, make_stream, mirrored

from raft_amd.params import RaftParams

pytestmark = pytest.mark.gpu

FORMS = ("device", "host")
DTYPES = dict(component=np.int32, degree=np.int32, comp_first=np.int32, comp_reads=np.int32, comp_bases=np.int64, comp_sides=np.int64)


@pytest.fixture(scope="module")
def eng():
    from raft_amd import engine
    e = engine.Engine(RaftParams(est_cov=3), device=0)
    yield e
    e.close()


def given_arrays(form, L, cols, strand, offset=False):
    import torch
    if form == "host":
        return [L] + list(cols) + [strand]

    def dev(a, dt):
        a = np.ascontiguousarray(a)
        if not offset:
            return torch.from_numpy(a).to("cuda:0")
        t = torch.zeros(a.size + 1, dtype=dt, device="cuda:0")[1:]         # 4 bytes (strand: 1 byte) off a 16-byte line
        t.copy_(torch.from_numpy(a))
        assert a.size == 0 or t.data_ptr() % 16 == (1 if dt == torch.uint8 else 4)
        return t
    return [dev(L, torch.int32)] + [dev(c, torch.int32) for c in cols] + [dev(strand, torch.uint8)]


def compare(got, want, tag):
    assert sorted(got) == sorted(PER_READ + PER_COMPONENT + ("summary", "kernel_seconds", "launches")), tag
    for k in PER_READ + PER_COMPONENT:
        g, w = got[k], want[k]
        assert g.dtype == DTYPES[k] and g.shape == w.shape, (tag, k, g.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, f"{tag}: {k} differs at {bad.size} places, first at {bad[0]}: got {g[bad[0]]} want {w[bad[0]]}"
    assert list(got["summary"]) == SUMMARY and got["summary"] == want["summary"], (tag, got["summary"], want["summary"])
    assert got["kernel_seconds"] >= 0.0 and got["launches"] == (0 if want["summary"]["n_reads"] == 0 else 6) + (1 if want["summary"]["n_records"] else 0), tag


def check(eng, L, cols, strand, H=1000, F=800, mask=KINDS_PROPER, symmetric=False, what="", forms=FORMS, offset=False, want=None):
    """Runs the call in every form and compares everything with the oracle (computed once) -> (the wanted dict, the last result)"""
    want = oracle(L, cols, strand, H, F, mask, symmetric) if want is None else want
    got = None
    for form in forms:
        tag = f"{what} ({form}, H={H}, F={F}, mask={mask}, symmetric={symmetric}, n_rec={cols[0].size}, n_reads={L.size})"
        got = eng.components(*given_arrays(form, L, cols, strand, offset), max_overhang=H, min_ratio_permille=F, kind_mask=mask, symmetric=symmetric)
        compare(got, want, tag)
    return want, got


def test_the_header_s_constants():
    from raft_amd import engine
    assert (engine.CC_KINDS_PROPER, engine.CC_KINDS_ALL) == (KINDS_PROPER, KINDS_ALL) == (0b111100, 0b111110)
    assert (T, STRIDE) == (1024, 2048 * 1024)


# ---- sizes
@pytest.mark.parametrize("n_rec", SIZES)
def test_every_number_of_records(eng, n_rec):
    rng = np.random.default_rng(n_rec + 11)
    L, cols, strand = make_stream(rng, 65 if n_rec < STRIDE else 3000, n_rec)
    want, _ = check(eng, L, cols, strand, what="sizes")
    check(eng, L, cols, strand, mask=KINDS_ALL, symmetric=True, what="sizes", forms=("device",))
    if n_rec >= 2 * T:
        assert want["summary"]["edge_records"] > 0 and want["summary"]["components"] < L.size


@pytest.mark.parametrize("n_reads", [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_every_number_of_reads(eng, n_reads):
    rng = np.random.default_rng(n_reads)
    # few records for many reads: components of every size from one up, and reads nobody names
    L, cols, strand = make_stream(rng, n_reads, n_reads // 2 + (3 if n_reads else 0)) if n_reads else (np.zeros(0, np.int32), [np.zeros(0, np.int32)] * 6, np.zeros(0, np.uint8))
    want, _ = check(eng, L, cols, strand, mask=KINDS_ALL, what="reads")
    if n_reads >= 63:
        assert 1 < want["summary"]["components"] < n_reads and want["summary"]["singletons"] > 0
    # ... and without records: every read alone
    none = [np.zeros(0, np.int32)] * 6
    want, got = check(eng, L, none, np.zeros(0, np.uint8), what="no records")
    assert want["summary"]["components"] == n_reads == want["summary"]["singletons"] and np.array_equal(got["component"], np.arange(n_reads))
    assert not got["degree"].any() and np.array_equal(got["comp_first"], np.arange(n_reads))


@pytest.mark.parametrize("n_rec", [1, 5, 257, 2 * T + 3])
def test_columns_off_the_16_byte_line(eng, n_rec):
    rng = np.random.default_rng(n_rec)
    L, cols, strand = make_stream(rng, 65, n_rec)
    check(eng, L, cols, strand, what="misaligned", forms=("device",), offset=True)


# ---- shapes that break a union: ascending, descending, shuffled
def path(n):
    return n, np.stack([np.arange(n - 1), np.arange(1, n)], axis=1)


def star(n, centre_is_query):
    leaves = np.arange(1, n)
    hub = np.full(n - 1, 0)
    return n, np.stack([hub, leaves] if centre_is_query else [leaves, hub], axis=1)


def cycle(n):
    return n, np.stack([np.arange(n), (np.arange(n) + 1) % n], axis=1)


def complete(n):
    a, b = np.triu_indices(n, 1)
    return n, np.stack([a, b], axis=1)


def two_halves(half, bridge_first):
    left, right = path(half)[1], path(half)[1] + half
    bridge = np.array([[half - 1, half]])
    return 2 * half, np.concatenate([bridge, left, right] if bridge_first else [left, right, bridge])


def many_components(largest):
    """Components of sizes 1 .. largest, each a path, their reads interleaved over the id range by a fixed permutation."""
    sizes = np.arange(1, largest + 1)
    n = int(sizes.sum())
    ids = np.random.default_rng(largest).permutation(n)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    pairs = [np.stack([ids[starts[k]:starts[k + 1] - 1], ids[starts[k] + 1:starts[k + 1]]], axis=1) for k in range(largest)]
    return n, np.concatenate(pairs)


SHAPES = {
    "path of 65537": lambda: path(65537),
    "star on one query": lambda: star(3000, True),
    "star on one target": lambda: star(3000, False),
    "cycle": lambda: cycle(5000),
    "complete graph on 64": lambda: complete(64),
    "two halves, the bridge last": lambda: two_halves(40000, False),
    "two halves, the bridge first": lambda: two_halves(40000, True),
    "1000 components of sizes 1..1000": lambda: many_components(1000),
    "every edge eight times": lambda: (lambda n, p: (n, np.repeat(p, 8, axis=0)))(*many_components(60)),
}
EXPECT = {"path of 65537": (1, 65537), "star on one query": (1, 3000), "star on one target": (1, 3000), "cycle": (1, 5000),
          "complete graph on 64": (1, 64), "two halves, the bridge last": (1, 80000), "two halves, the bridge first": (1, 80000),
          "1000 components of sizes 1..1000": (1000, 1000), "every edge eight times": (60, 60)}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_shapes_that_break_a_union(eng, shape):
    n_reads, pairs = SHAPES[shape]()
    L, cols, strand = edge_stream(n_reads, pairs)
    want = oracle(L, cols, strand)
    assert (want["summary"]["components"], want["summary"]["largest_reads"]) == EXPECT[shape], want["summary"]
    assert want["summary"]["edge_records"] == len(pairs)
    n = len(pairs)
    orders = {"ascending": np.arange(n), "descending": np.arange(n)[::-1], "shuffled": np.random.default_rng(7).permutation(n)}
    for name, order in orders.items():
        c, s = reordered(cols, strand, order)
        check(eng, L, c, s, what=f"{shape}, {name}", forms=FORMS if name == "shuffled" else ("device",), want=want)


# ---- the mask
@pytest.mark.parametrize("mask", [1 << 1, 1 << 2, 1 << 3, 1 << 4, 1 << 5, KINDS_PROPER, KINDS_ALL])
def test_every_mask_on_a_stream_with_every_kind(eng, mask):
    rng = np.random.default_rng(41)
    L, cols, strand = make_stream(rng, 3000, 2 * T + 3)
    from test_gpu_overlap_ends import want_kinds
    assert set(np.unique(want_kinds(L, cols, strand, 1000, 800))) == set(range(7))
    want, _ = check(eng, L, cols, strand, mask=mask, what="mask")
    assert 0 < want["summary"]["edge_records"] < cols[0].size
    check(eng, L, cols, strand, mask=mask, symmetric=True, what="mask", forms=("device",))


def test_one_component_under_all_and_several_under_proper(eng):
    """Four paths of containments, bridged by internal matches, with self and invalid records between reads that stay apart."""
    rng = np.random.default_rng(2)
    n_reads, size = 400, 80
    L = np.full(n_reads, 9000, np.int32)
    rows = []
    for g in range(4):
        for r in range(g * size, (g + 1) * size - 1):
            rows.append((r, 0, 9000, r + 1, 0, 9000, 0))                  # both whole: a containment
    for g in range(3):
        rows.append(((g + 1) * size - 1, 4000, 4500, (g + 1) * size, 3000, 3500, 1))     # inside both: internal
    for r in range(320, 399):
        rows.append((r, 0, 500, r, 8500, 9000, 0))                         # a read against itself
        rows.append((r, 10, 10, r + 1, 0, 9000, 0))                        # invalid: empty on the query
        rows.append((r, 0, 9000, r + 1, 0, 9001, 1))                       # invalid: beyond the target's end
    rows = np.array(rows, np.int64)[rng.permutation(len(rows))]
    cols = [np.ascontiguousarray(rows[:, k].astype(np.int32)) for k in range(6)]
    strand = np.ascontiguousarray(rows[:, 6].astype(np.uint8))
    both, _ = check(eng, L, cols, strand, mask=KINDS_ALL, what="bridged")
    proper, _ = check(eng, L, cols, strand, mask=KINDS_PROPER, what="bridged")
    inner, _ = check(eng, L, cols, strand, mask=1 << 1, what="bridged")
    assert both["summary"]["components"] == 1 + 80 and both["summary"]["largest_reads"] == 320
    assert proper["summary"]["components"] == 4 + 80 and proper["summary"]["largest_reads"] == 80 and proper["summary"]["singletons"] == 80
    assert inner["summary"]["components"] == 400 - 3 and inner["summary"]["edge_records"] == 3


# ---- the order of the records
def test_five_orders_of_one_stream_give_the_same_bytes(eng):
    rng = np.random.default_rng(77)
    L, cols, strand = make_stream(rng, 20000, 40 * T + 5)
    want, first = check(eng, L, cols, strand, mask=KINDS_ALL, what="order 0", forms=("device",))
    assert 1 < want["summary"]["components"] < 20000 and want["summary"]["largest_reads"] > 1000
    for k in range(1, 6):
        c, s = reordered(cols, strand, rng.permutation(cols[0].size))
        got = eng.components(*given_arrays("device", L, c, s), kind_mask=KINDS_ALL)
        for name in PER_READ + PER_COMPONENT:
            assert got[name].tobytes() == first[name].tobytes(), (k, name)
        assert got["summary"] == first["summary"], k


# ---- symmetric
@pytest.mark.parametrize("mask", [KINDS_PROPER, KINDS_ALL])
def test_a_mirrored_stream_counted_on_its_query_sides_is_its_half_counted_on_both(eng, mask):
    rng = np.random.default_rng(mask)
    L, cols, strand = make_stream(rng, 3000, 2 * T + 3)
    half, _ = check(eng, L, cols, strand, mask=mask, what="half")
    full_cols, full_strand = mirrored(cols, strand)
    full, _ = check(eng, L, full_cols, full_strand, mask=mask, symmetric=True, what="mirrored")
    for k in PER_READ + PER_COMPONENT:
        assert np.array_equal(full[k], half[k]), k
    assert full["summary"]["edge_records"] == 2 * half["summary"]["edge_records"]
    assert np.array_equal(edge_mask(L, full_cols, full_strand, 1000, 800, mask), np.tile(edge_mask(L, cols, strand, 1000, 800, mask), 2))


# ---- errors
def raw_call(eng, form, L, cols, strand, H=1000, F=800, mask=KINDS_PROPER, symmetric=0, outs=None, n_reads=None, n_rec=None, summary=None):
    """The entry point itself, with the caller's output arrays (six, or None: all NULL) -> (code, error_index, the context's message)"""
    import torch
    from raft_amd import engine
    lib = engine.load_side_library("cc")
    arrays = [L] + list(cols) + [strand]
    if form == "device":
        held = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in arrays]
        eng.use_torch_stream()
        fn = lib.raft_hip_components_device
    else:
        held, fn = arrays, lib.raft_hip_components_host
    p = [engine.M.ptr(a) for a in held]
    err = C.c_int64(-5)
    rc = fn(eng._ctx, L.size if n_reads is None else n_reads, p[0], cols[0].size if n_rec is None else n_rec, *p[1:], H, F, mask, symmetric,
            *[engine.M.ptr(o) for o in (outs or [None] * 6)], None if summary is None else C.byref(summary), C.byref(err), None, None)
    return rc, err.value, eng._lib.raft_hip_last_error(eng._ctx).decode()


def marked_outputs(n):
    return [np.full(n, -9, np.int32) for _ in range(4)] + [np.full(n, -9, np.int64) for _ in range(2)]


@pytest.mark.parametrize("form", FORMS)
def test_the_first_bad_id_is_reported_and_the_outputs_stay(eng, form):
    from raft_amd import engine
    rng = np.random.default_rng(3)
    n = 6 * T + 3                                                          # (six workgroups)
    L, cols, strand = make_stream(rng, 65, n)
    for bad_q, bad_t in (([5500, 700], [900]), ([1500], [40, 6000]), ([n - 1], []), ([], [0]), ([5], [5])):
        c = [x.copy() for x in cols]
        c[0][bad_q] = [65, -1][: len(bad_q)]
        c[3][bad_t] = [-2147483648, 65][: len(bad_t)]
        outs, sm = marked_outputs(65), engine._CcSummary(n_reads=-9)
        rc, index, message = raw_call(eng, form, L, c, strand, outs=outs, summary=sm)
        assert rc == engine.ERR_READ_ID and index == min(bad_q + bad_t), (form, bad_q, bad_t, rc, index)
        assert message.startswith("components:")
        assert all(np.all(o == -9) for o in outs) and sm.n_reads == -9
        with pytest.raises(engine.RaftError) as e:
            eng.components(L, *c, strand)
        assert e.value.code == engine.ERR_READ_ID and e.value.index == min(bad_q + bad_t)
    outs = marked_outputs(65)
    rc, index, _ = raw_call(eng, form, L, cols, strand, outs=outs)
    want = oracle(L, cols, strand)
    C_ = want["summary"]["components"]
    assert rc == engine.OK and index == -1
    assert np.array_equal(outs[0], want["component"]) and np.array_equal(outs[1], want["degree"])
    for o, k in zip(outs[2:], PER_COMPONENT):
        assert np.array_equal(o[:C_], want[k]) and np.all(o[C_:] == -9), k       # (what lies behind the C entries is left as it was)


def test_the_refusals(eng):
    from raft_amd import engine
    rng = np.random.default_rng(1)
    L, cols, strand = make_stream(rng, 65, 100)
    outs = marked_outputs(65)
    for form in FORMS:
        for H, F in ((-1, 800), (1000, -1), (1000, 1001), (-2147483648, 0)):
            rc, _, message = raw_call(eng, form, L, cols, strand, H=H, F=F, outs=outs)
            assert rc == engine.ERR_PARAM and message.startswith("components:"), (form, H, F, rc, message)
        for mask in (0, 1, 64, 63, 62 | 128, -1, 1 << 6, -2147483648):
            rc, _, message = raw_call(eng, form, L, cols, strand, mask=mask, outs=outs)
            assert rc == engine.ERR_PARAM and message.startswith("components: kind_mask"), (form, mask, rc, message)
        for kw in ({"n_rec": -1}, {"n_reads": -1}):
            rc, _, message = raw_call(eng, form, L, cols, strand, outs=outs, **kw)
            assert rc == engine.ERR_PARAM and message.startswith("components:"), (form, kw)
        for missing in range(8):
            arrays = [L] + list(cols) + [strand]
            arrays[missing] = None
            rc, _, message = raw_call(eng, form, arrays[0], arrays[1:7], arrays[7], outs=outs, n_reads=65, n_rec=100)
            assert rc == engine.ERR_PARAM and message.startswith("components:"), (form, missing)
        assert all(np.all(o == -9) for o in outs)
    with pytest.raises(engine.RaftError) as e:
        eng.components(L, *cols, strand, kind_mask=0)
    assert e.value.code == engine.ERR_PARAM and "components" in str(e.value)
    with pytest.raises(ValueError):
        eng.components(L, *cols, None)
    check(eng, L, cols, strand, what="after the refusals")


@pytest.mark.parametrize("form", FORMS)
def test_every_output_may_be_null(eng, form):
    from raft_amd import engine
    rng = np.random.default_rng(8)
    L, cols, strand = make_stream(rng, 300, T + 1)
    want = oracle(L, cols, strand)
    sm = engine._CcSummary()
    rc, index, _ = raw_call(eng, form, L, cols, strand, summary=sm)
    assert rc == engine.OK and index == -1 and {k: getattr(sm, k) for k in SUMMARY} == want["summary"]
    for only in range(6):
        outs = [None] * 6
        outs[only] = marked_outputs(300)[only]
        rc, _, _ = raw_call(eng, form, L, cols, strand, outs=outs)
        k = (PER_READ + PER_COMPONENT)[only]
        assert rc == engine.OK and np.array_equal(outs[only][:want[k].size], want[k]), k


def test_calls_of_falling_and_rising_size_on_one_context(eng):
    rng = np.random.default_rng(9)
    for n_reads, n_rec in ((5000, 4 * T + 1), (2, 5), (65, T + 1), (1, 3), (5000, 8 * T + 7), (65, 0), (5000, 2 * T)):
        L, cols, strand = make_stream(rng, n_reads, n_rec)
        check(eng, L, cols, strand, what="sequence", symmetric=n_rec % 2 == 0, mask=KINDS_ALL if n_rec % 3 == 0 else KINDS_PROPER)
