"""GPU: raft_hip_unitigs_device / _host (raft_amd/csrc/unitig.hpp, unitig_lib.hip) -- every output array, the summary, the launch
count and the error paths, equal to a sequential Python walk over the same arrays (tests/unitig_testlib.py), in the device form and
the host form.  The tables are made directly (chains, cycles, singletons and skipped reads by construction), and once from a record
stream through ``Engine.best_overlaps``."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from raft_testlib import ROOT
from unitig_testlib import PER_READ, PER_UNITIG, SUMMARY, first_bad_read, make_table, rounds_of, walk

from raft_amd.params import RaftParams

pytestmark = pytest.mark.gpu

FORMS = ("device", "host")
CLASSES = ("reverse_edges", "cycles", "singletons", "skipped", "chain_of_1024", "offset_past_2_32")


def _constant(name):
    text = open(os.path.join(ROOT, "raft_amd", "csrc", "unitig.hpp")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


# beyond kUtgMaxBlocks workgroups of kUtgThreads lanes the grids stride: a lane per read in the init, place and emit kernels, a lane
# per half-edge in the rounds
STRIDE = _constant("kUtgThreads") * _constant("kUtgMaxBlocks")
SIZES = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, STRIDE + 1]


def test_the_constants_are_the_expected_ones():
    assert STRIDE == 256 * 2048


def launches_of(n_reads, cycles):
    """init + the rounds, (mark + init + the rounds), place, two of the scan, emit"""
    if n_reads == 0:
        return 0
    return (1 + rounds_of(n_reads)) * (2 if cycles else 1) + (1 if cycles else 0) + 4


@pytest.fixture(scope="module")
def eng():
    from raft_amd import engine
    e = engine.Engine(RaftParams(est_cov=3), device=0)
    yield e
    e.close()


TALLY = dict.fromkeys(CLASSES, 0)
_seen = set()


def count_classes(what, table, w):
    """What the case holds of every class, counted on the oracle's side, once per case."""
    if what in _seen:
        return
    _seen.add(what)
    L, partner, span, flags = table
    TALLY["reverse_edges"] += int((((flags & 3) == 3).sum() + ((flags & 12) == 12).sum()))
    TALLY["cycles"] += w["summary"]["circular"]
    TALLY["singletons"] += w["summary"]["singletons"]
    TALLY["skipped"] += w["summary"]["reads_skipped"]
    TALLY["chain_of_1024"] += int((w["utg_reads"] >= 1024).sum())
    TALLY["offset_past_2_32"] += int((w["offset"] >= 2 ** 32).sum())


def check(eng, table, what, forms=FORMS, offset=False):
    """Runs the call in every form and compares every array, the summary and the launch count with the walk; -> the walk's result."""
    import torch
    L, partner, span, flags = table
    n = L.size
    assert first_bad_read(L, partner, span, flags) == -1, what
    w = walk(L, partner, span, flags)
    count_classes(what, table, w)
    for form in forms:
        if form == "device":
            def dev(a, dt):
                a = np.ascontiguousarray(a)
                if not offset:
                    return torch.from_numpy(a).to("cuda:0")
                t = torch.zeros(a.size + 1, dtype=dt, device="cuda:0")[1:]     # 4 bytes (flags: 1 byte) off a 16-byte line
                t.copy_(torch.from_numpy(a.reshape(-1)))
                assert a.size == 0 or t.data_ptr() % 16 == (1 if dt == torch.uint8 else 4)
                return t
            given = [dev(L, torch.int32), dev(partner, torch.int32), dev(span, torch.int32), dev(flags, torch.uint8)]
        else:
            given = [L, partner.reshape(-1) if n % 2 else partner, span, flags]           # [2n] and [n, 2] are both taken
        tag = f"{what} ({form}, n_reads={n})"
        got = eng.unitigs(*given)
        n_utg, placed = w["summary"]["unitigs"], n - w["summary"]["reads_skipped"]
        shapes = dict(order=(np.int32, placed), utg_off=(np.int64, n_utg + 1))
        shapes.update({k: (dt, n) for k, dt in PER_READ})
        shapes.update({k: (dt, n_utg) for k, dt in PER_UNITIG})
        for key, (dt, size) in shapes.items():
            assert got[key].dtype == dt and got[key].shape == (size,), (tag, key, got[key].shape)
            bad = np.flatnonzero(got[key] != w[key])
            assert bad.size == 0, f"{tag}: {key} differs at {bad.size} places, first at {bad[0]}: got {got[key][bad[0]]} want {w[key][bad[0]]}"
        assert got["summary"] == w["summary"] and tuple(got["summary"]) == SUMMARY, (tag, got["summary"], w["summary"])
        assert got["launches"] == launches_of(n, w["summary"]["circular"] > 0) == eng.last_unitigs_launches, (tag, got["launches"])
        assert got["kernel_seconds"] >= 0.0
    return w


def random_chains(rng, n_reads):
    """Chains and cycles of random lengths over about three quarters of the reads"""
    chains, left = [], (3 * n_reads + 3) // 4
    while left > 0:
        k = int(min(left, rng.integers(1, max(2, n_reads // 3) + 1)))
        chains.append((k, bool(k >= 2 and rng.random() < 0.4)))
        left -= k
    return chains


def table_of_size(n_reads):
    rng = np.random.default_rng(n_reads + 11)
    if n_reads > 100000:                  # the stride: most reads stand alone, so that the walk in Python stays short
        chains = [(2049, False), (1024, True), (2, True), (3, False)] + [(int(k), bool(k % 2)) for k in rng.integers(2, 40, 60)]
        return make_table(rng, n_reads, chains, skipped=1000)
    chains = random_chains(rng, n_reads)
    return make_table(rng, n_reads, chains, skipped=(n_reads - sum(k for k, _ in chains)) // 2)


@pytest.mark.parametrize("n_reads", SIZES)
def test_every_size(eng, n_reads):
    check(eng, table_of_size(n_reads), f"size {n_reads}")


def test_sizes_in_falling_order_on_one_context(eng):
    """State that a call leaves behind in the context's buffers shows up here: the ranking's two halves, the cut flags, the totals."""
    for n_reads in reversed(SIZES[:-1]):
        check(eng, table_of_size(n_reads), f"size {n_reads}")
    rng = np.random.default_rng(2)
    check(eng, make_table(rng, 300, [(64, True), (5, True)]), "cycles, then none: the cut flags of the call before")
    check(eng, make_table(rng, 300, [(64, False), (5, False)]), "no cycle behind a call with cycles")


@pytest.mark.parametrize("k", range(1, 12))
def test_chain_lengths_around_every_power_of_two(eng, k):
    """Chains of 1, 2, 3 and 2^k - 1, 2^k, 2^k + 1 reads: a walk that ends in round k, one before and one behind it"""
    rng = np.random.default_rng(k)
    lengths = [1, 2, 3, 2 ** k - 1, 2 ** k, 2 ** k + 1]
    n_reads = sum(lengths) + 7
    assert rounds_of(n_reads) >= k + 1
    w = check(eng, make_table(rng, n_reads, [(x, False) for x in lengths if x >= 1], skipped=3), f"chains around 2^{k}")
    assert w["summary"]["circular"] == 0 and w["summary"]["longest_reads"] == 2 ** k + 1


@pytest.mark.parametrize("n_reads", [2, 3, 4, 64, 65, 1024, 4097])
@pytest.mark.parametrize("circular", [False, True])
def test_one_component_over_all_reads(eng, n_reads, circular):
    """One chain over all reads of the case: the walks that end last.  One cycle over all of them: the minimum needs every round, and
    the cut and the second ranking run."""
    rng = np.random.default_rng(n_reads + (1 if circular else 0))
    w = check(eng, make_table(rng, n_reads, [(n_reads, circular)]), f"one {'cycle' if circular else 'chain'} over all reads")
    assert w["summary"]["unitigs"] == 1 and w["summary"]["circular"] == (1 if circular else 0) and w["utg_reads"][0] == n_reads


@pytest.mark.parametrize("orients", [[0, 0], [0, 1], [1, 0], [1, 1]])
def test_cycles_of_two_in_both_strand_forms(eng, orients):
    """a3-b5 / b3-a5 on '+', a3-b3 / a5-b5 on '-'"""
    rng = np.random.default_rng(5)
    table = make_table(rng, 9, [(2, True), (2, True)], orients=[orients, orients[::-1]], skipped=2)
    w = check(eng, table, f"cycles of two, orientations {orients}")
    assert w["summary"]["circular"] == 2 and ((table[3] & 3) == 3).any() == (orients[0] != orients[1])


@pytest.mark.parametrize("k", [3, 4, 8, 64, 256, 2048])
def test_cycles(eng, k):
    rng = np.random.default_rng(k)
    w = check(eng, make_table(rng, 3 * k + 50, [(k, True), (5, False), (k, True), (k, False), (2, True)], skipped=10), f"cycles of {k}")
    assert w["summary"]["circular"] == 3


def test_the_second_ranking_runs_only_with_a_cycle(eng):
    rng = np.random.default_rng(8)
    for chains, cycles in (([(100, False), (7, False)], False), ([(100, False), (2, True)], True), ([], False)):
        got = eng.unitigs(*make_table(rng, 200, chains, skipped=5))
        assert got["summary"]["circular"] == (1 if cycles else 0)
        assert got["launches"] == launches_of(200, cycles) and launches_of(200, True) - launches_of(200, False) == 2 + rounds_of(200)


def test_offsets_past_2_32(eng):
    rng = np.random.default_rng(6)
    top = 2 ** 31 - 1
    table = make_table(rng, 40, [(12, False), (9, True), (2, False)], skipped=2, len_range=(top - 1000, top), span_max=5000)
    w = check(eng, table, "read lengths near INT32_MAX")
    assert w["offset"].max() > 2 ** 34 and w["utg_length"].max() > 2 ** 34 and w["summary"]["total_length"] > 2 ** 35


@pytest.mark.parametrize("n_reads", [1, 5, 257, 5000])
def test_tensors_off_the_16_byte_line(eng, n_reads):
    rng = np.random.default_rng(n_reads)
    check(eng, make_table(rng, n_reads, random_chains(rng, n_reads)), "misaligned", forms=("device",), offset=True)


def test_negative_lengths_count_as_zero(eng):
    rng = np.random.default_rng(4)
    L, partner, span, flags = make_table(rng, 50, [(10, False), (4, True)], skipped=3)
    alone = np.flatnonzero((flags & 10) == 0)
    L[alone[:5]] = [-1, -2147483648, -7, 0, -1]
    w = check(eng, (L, partner, span, flags), "lengths below 0")
    assert (w["utg_length"] == 0).sum() >= 2


# ---- the error paths
def raw_call(eng, form, table, out, n_reads=None, summary=None):
    """The entry point itself, with the caller's output arrays -> (code, error_index, the context's message)"""
    import torch
    from raft_amd import engine
    lib = engine.load_side_library("utg")
    if form == "device":
        held = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in table]
        eng.use_torch_stream()
        fn = lib.raft_hip_unitigs_device
    else:
        held, fn = [None if a is None else np.ascontiguousarray(a) for a in table], lib.raft_hip_unitigs_host
    err = C.c_int64(-5)
    rc = fn(eng._ctx, table[0].size if n_reads is None else n_reads, *[engine.M.ptr(a) for a in held], *[engine.M.ptr(a) for a in out],
            None if summary is None else C.byref(summary), C.byref(err), None, None)
    return rc, err.value, eng._lib.raft_hip_last_error(eng._ctx).decode()


OUT = (("unitig", np.int32), ("index", np.int32), ("offset", np.int64), ("orient", np.uint8), ("order", np.int32), ("utg_off", np.int64),
       ("utg_reads", np.int32), ("utg_length", np.int64), ("utg_circular", np.uint8))


def outputs(n_reads):
    return [np.full(n_reads + 1, 9, dt) for _, dt in OUT]


def untouched(out, summary=None):
    return all(np.all(a == 9) for a in out) and (summary is None or summary.reads_in == -9)


def broken_tables():
    """One table per violated condition, each from a sound one: (what, the table)"""
    rng = np.random.default_rng(12)
    n = 70
    sound = make_table(rng, n, [(20, False), (6, True), (9, False)], skipped=4, junk=False)
    L, partner, span, flags = sound
    ends = [(r, e) for r in range(n) for e in range(2) if (flags[r] >> (2 * e)) & 2]
    r, e = ends[len(ends) // 2]
    p, rev = partner[r, e], (flags[r] >> (2 * e)) & 1
    pe = e if rev else 1 - e
    skipped = int(np.flatnonzero(flags & 16)[0])
    cases = []

    def case(what, edit):
        t = [a.copy() for a in sound]
        edit(*t)
        cases.append((what, tuple(t)))

    case("r is SKIPPED", lambda L, P, S, F: F.__setitem__(r, F[r] | 16))
    case("p below 0", lambda L, P, S, F: P.__setitem__((r, e), -1))
    case("p == n_reads", lambda L, P, S, F: P.__setitem__((r, e), n))
    case("p far outside", lambda L, P, S, F: P.__setitem__((r, e), 2 ** 31 - 1))
    case("p == r", lambda L, P, S, F: P.__setitem__((r, e), r))
    case("p is SKIPPED", lambda L, P, S, F: P.__setitem__((r, e), skipped))
    case("p has no MUTUAL at E'", lambda L, P, S, F: F.__setitem__(p, int(F[p]) & (255 ^ (2 << (2 * pe)))))
    case("the REV bits differ", lambda L, P, S, F: F.__setitem__(p, F[p] ^ (1 << (2 * pe))))
    case("the partner does not lead back", lambda L, P, S, F: P.__setitem__((p, pe), (r + 1) % n))
    case("the spans differ", lambda L, P, S, F: S.__setitem__((p, pe), S[p, pe] + 1))
    case("span 0", lambda L, P, S, F: (S.__setitem__((r, e), 0), S.__setitem__((p, pe), 0)))
    case("span above a length", lambda L, P, S, F: (S.__setitem__((r, e), min(L[r], L[p]) + 1), S.__setitem__((p, pe), min(L[r], L[p]) + 1)))
    case("span above a length that counts as 0", lambda L, P, S, F: L.__setitem__(r, -5))
    case("two bad reads", lambda L, P, S, F: (P.__setitem__(ends[-1], -3), P.__setitem__(ends[0], n + 7)))
    return sound, cases


@pytest.mark.parametrize("form", FORMS)
def test_every_violated_condition_is_reported_and_the_outputs_stay(eng, form):
    from raft_amd import engine
    sound, cases = broken_tables()
    n = sound[0].size
    assert len(cases) == 14
    for what, table in cases:
        want = first_bad_read(*table)
        assert want >= 0, what
        out, summary = outputs(n), engine._UtgSummary(reads_in=-9)
        rc, index, message = raw_call(eng, form, table, out, summary=summary)
        assert rc == engine.ERR_READ_ID and index == want, (form, what, rc, index, want)
        assert message.startswith("unitigs:") and untouched(out, summary), (form, what, message)
        with pytest.raises(engine.RaftError) as e:
            eng.unitigs(*table)
        assert e.value.code == engine.ERR_READ_ID and e.value.index == want
    out = outputs(n)
    rc, index, _ = raw_call(eng, form, sound, out)
    w = walk(*sound)
    assert rc == engine.OK and index == -1
    for (key, _), a in zip(OUT, out):
        assert np.array_equal(a[:w[key].size], w[key]) and np.all(a[w[key].size:] == 9), key       # ... and nothing behind what the call owes


def test_the_refusals(eng):
    from raft_amd import engine
    rng = np.random.default_rng(1)
    table = make_table(rng, 65, [(20, False), (3, True)], skipped=5)
    out = outputs(65)
    for form in FORMS:
        rc, _, message = raw_call(eng, form, table, out, n_reads=-1)
        assert rc == engine.ERR_PARAM and message.startswith("unitigs:"), (form, rc, message)
        rc, _, message = raw_call(eng, form, table, out, n_reads=-2147483648)
        assert rc == engine.ERR_PARAM and message.startswith("unitigs:"), (form, rc, message)
        for n_reads in (2 ** 30, 2 ** 31 - 1):
            rc, _, message = raw_call(eng, form, table, out, n_reads=n_reads)
            assert rc == engine.ERR_TOO_LARGE and message.startswith("unitigs:"), (form, n_reads, rc, message)
        for missing in range(4):
            t = list(table)
            t[missing] = None
            rc, _, message = raw_call(eng, form, t, out, n_reads=65)
            assert rc == engine.ERR_PARAM and message.startswith("unitigs:"), (form, missing)
        assert untouched(out)
        # n_reads == 0 is valid, with or without arrays: U = 0
        for t in ((None,) * 4, table):
            o, summary = outputs(0), engine._UtgSummary(reads_in=-9)
            rc, index, _ = raw_call(eng, form, t, o, n_reads=0, summary=summary)
            assert rc == engine.OK and index == -1 and summary.reads_in == 0 and summary.unitigs == 0 and o[5][0] == 0
    with pytest.raises(ValueError):
        eng.unitigs(table[0], table[1], table[2], None)
    with pytest.raises(ValueError):
        eng.unitigs(table[0], table[1][:-1], table[2], table[3])
    check(eng, table, "after the refusals")


def test_behind_best_overlaps_on_its_tensors(eng):
    """A record stream -> Engine.best_overlaps (device) -> Engine.unitigs on the tensors of that result, against the walk over the
    restatement's arrays."""
    import torch
    from test_gpu_best_overlaps import status_mask, want_best
    from test_gpu_overlap_ends import make_stream
    for n_reads, n_rec in ((65, 700), (5000, 40000)):
        rng = np.random.default_rng(n_reads)
        L, cols, strand = make_stream(rng, n_reads, n_rec)
        skip = status_mask(L, cols, strand, 1000, 800, False)
        dev = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in [L] + list(cols) + [strand, skip]]
        best = eng.best_overlaps(*dev[:8], skip=dev[8])
        w_partner, w_span, w_flags, _ = want_best(L, cols, strand, 1000, 800, False, skip)
        assert np.array_equal(best["partner"], w_partner) and np.array_equal(best["flags"], w_flags)
        on_device = [torch.from_numpy(best[k]).to("cuda:0") for k in ("partner", "span", "flags")]
        got = eng.unitigs(dev[0], *on_device)
        w = walk(L, w_partner, w_span, w_flags)
        for key in [k for k, _ in OUT]:
            assert np.array_equal(got[key], w[key]), (n_reads, key)
        assert got["summary"] == w["summary"]
        assert w["summary"]["unitigs"] < n_reads - w["summary"]["reads_skipped"], "the stream forms no chain at all"


def test_zz_the_cases_hold_every_class(eng):
    """A class that the cases do not fill would make the comparisons say nothing about it.  Counted on the oracle's side while the
    cases above ran (this test is the file's last); run alone, it makes the cases it needs itself."""
    if not _seen:
        rng = np.random.default_rng(3)
        top = 2 ** 31 - 1
        check(eng, make_table(rng, 1500, [(1100, False), (30, True)], skipped=20), "tally: a long chain")
        check(eng, make_table(rng, 30, [(12, False)], len_range=(top - 1000, top), span_max=5000), "tally: long reads")
    assert all(TALLY[c] > 0 for c in CLASSES), TALLY
