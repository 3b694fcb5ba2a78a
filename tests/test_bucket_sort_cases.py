"""CPU: the cases that tests/test_gpu_bucket_sort.py runs through the general bucketing's sorts (sort_pairs.hpp:101-423,
bucket.hpp:353-604, engine.hip bucket_sides) -- and what keeps them honest.

The constants the cases are laid on are read back from the sources, so that a retune fails here instead of moving the tile, segment and
gap edges away from the cases.  From the cases alone a census counts which structural classes every case falls in -- the last tile's
fill, tile counts that are no multiple of eight, the table scan's segment length L, the digit passes, a tile owned by one digit, half of
all slots without a side, runs of 31 and 32 reads without sides, the gap list below and above its capacity -- and fails on an empty
class.  sides_reference, the plain statement of what the sorts must produce, is pinned to a hand-written example, to the oracle's
interval count on every pass-level set and, through a numpy pileup of its output, to the oracle's coverage; the comparator is shown to
fail and to say where.  The conditions on the pass-level sets (repeats, reads in several fragments, symmetry, 16-bit window indices)
are checked with the oracle."""
import os
import re

import numpy as np
import pytest
import raft_testlib as T
from raft_testlib import (GAP_INLINE, GAP_LIST, ITEM_TILE, PAIR_TILE, ROOT, RS_SEGS, SORT_GROUPS, assert_same_sides, bucket_pass_cases,
                          bucket_sort_cases, census_classes, oracle_run, side_keys, sides_first_difference, sides_pileup, sides_reference,
                          sort_census)

CSRC = os.path.join(ROOT, "raft_amd", "csrc")


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def test_the_constants_the_cases_are_built_on():
    sp, bk, en = _src("sort_pairs.hpp"), _src("bucket.hpp"), _src("engine.hip")

    def one(pattern, text):
        m = re.findall(pattern, text)
        assert len(m) == 1, (pattern, m)
        return m[0]
    assert int(one(r"#define RAFT_RS_WAVES (\d+)\b", sp)) == T.RS_WAVES == 4
    one(r"kRsThreads = 64 \* kRsWaves\b", sp)
    one(r"kTile = kRsThreads \* IPT\b", sp)
    assert one(r"struct RsIpt \{ static constexpr int v = sizeof\(V\) == 8 \? (\d+) : (\d+); \}", sp) == ("16", "32")
    assert int(one(r"constexpr int kRsItemsIpt = (\d+);", sp)) == T.ITEM_IPT == 32
    assert int(one(r"constexpr int kRsSegs = (\d+);", sp)) == RS_SEGS == 256
    assert one(r"constexpr int kGapInline = (\d+), kGapList = (\d+);", bk) == ("32", "1024")
    assert (GAP_INLINE, GAP_LIST) == (32, 1024)
    one(r"if \(hi - lo >= kGapInline && gaps\)", bk)
    assert one(r"const bool parted = cap_iv >= \(1LL << (\d+)\)", en) == "20" and T.SORT_THRESHOLD == 1 << 20
    assert one(r"wide = wide \|\| first > (\d+)u \|\| last1 > (\d+)u;", bk) == ("65535", "65535")
    assert (PAIR_TILE, ITEM_TILE) == (64 * 4 * 16, 64 * 4 * 32) == (4096, 8192)


def _require(classes, want, what):
    missing = [k for k in want if not classes.get(k)]
    assert not missing, f"{what}: no case in the classes {missing}"


GAP_CLASSES = ([("between", g) for g in (31, 32)] + [("leading", g) for g in (31, 32)] + [("trailing", g) for g in (31, 32)]
               + [("listed", "<=1024"), ("listed", ">1024")])


def test_census_of_the_direct_cases():
    cases = bucket_sort_cases()
    assert len({c.name for c in cases}) == len(cases) and {c.group for c in cases} == set(SORT_GROUPS)
    cen = {}
    for c in cases:
        name, n_reads, cols, sym = c
        assert name == c.name and all(a.dtype == np.int32 for a in cols)
        cen[name] = sort_census(n_reads, side_keys(n_reads, cols[0], cols[3], sym), PAIR_TILE)
        assert cen[name]["n_ent"] == c.n_ent
    classes = census_classes(cen, PAIR_TILE)
    _require(classes, [("n_valid_last", v) for v in (1, 63, 64, 65, "full")] + [("tiles_mod8", "nonzero")] + [("L", v) for v in (1, 2, 3)]
             + [("passes", v) for v in (1, 2, 3, 4)] + [("whole_tile_one_digit", True), ("absent_share", ">=0.5")] + GAP_CLASSES, "direct cases")
    # ... and the lattice of the slot counts itself, by symmetry: a stream that is not symmetric has an even number of slots
    have = {(c.symmetric, c.n_ent) for c in cases if c.group.startswith("sizes")}
    for n in T.SORT_SIZES:
        assert (True, n) in have and (n % 2 == 1 or (False, n) in have), n
    for t in (7, 8, 9, 255, 256, 257):
        assert {t * 4096 - 1, t * 4096, t * 4096 + 1} <= set(T.SORT_SIZES)
    assert {0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 513 * 4096} <= set(T.SORT_SIZES)
    assert cen["sizes_sym/n_ent=1048576"]["L"] == 1 and cen["sizes_sym/n_ent=1048577"]["L"] == 2      # 256 tiles, 257 tiles
    assert {c.n_reads for c in cases if c.group == "widths"} == set(T.SORT_WIDTHS)
    # the gap list one short of full, exactly full, overflowing; one long gap; a lone read at either end
    assert [cen[f"gaps/gaps_of_40={g}"]["listed"] for g in (1023, 1024, 1100)] == [1023, 1024, 1100]
    assert cen["gaps/one_gap=1e6"]["between"] == {10 ** 6}
    assert cen["gaps/last_read_only"]["leading"] == 69999 and cen["gaps/first_read_only"]["trailing"] == 69999
    # every distribution at one, two and three passes, over more than one tile
    for d in T.SORT_DISTS:
        assert sorted(cen[f"dists/{d}/n_reads={w}"]["passes"] for w in T.SORT_DIST_WIDTHS) == [1, 2, 3]
        assert all(cen[f"dists/{d}/n_reads={w}"]["n_tiles"] > 1 for w in T.SORT_DIST_WIDTHS)
    for w in T.SORT_DIST_WIDTHS:
        assert cen[f"dists/one_read/n_reads={w}"]["whole_tile_one_digit"] and cen[f"dists/self/n_reads={w}"]["absent_share"] == 0.5
        assert cen[f"dists/no_self/n_reads={w}"]["absent_share"] == 0.0
    # a context meets its sizes in both directions
    for g in SORT_GROUPS:
        n = [c.n_ent for c in cases if c.group == g]
        assert any(a > b for a, b in zip(n, n[1:])) and any(a < b for a, b in zip(n, n[1:])), g


def test_census_of_the_pass_cases():
    """With ITEM_TILE tiles.  A stream that is not symmetric has an even number of slots, so the short last tiles are 2, 64 and 66."""
    cen = {}
    for c in bucket_pass_cases():
        name, p, cols = c
        cen[name] = sort_census(cols[0].size, side_keys(cols[0].size, cols[1], cols[4], c.symmetric), ITEM_TILE)
    classes = census_classes(cen, ITEM_TILE)
    _require(classes, [("n_valid_last", v) for v in (2, 64, 66, "full")] + [("tiles_mod8", "nonzero")] + [("L", v) for v in (1, 2)]
             + [("passes", v) for v in (1, 2, 3, 4)] + [("whole_tile_one_digit", True), ("absent_share", ">=0.5")] + GAP_CLASSES, "pass cases")
    n_ent = {k: v["n_ent"] for k, v in cen.items()}
    assert (n_ent["thr_below"], n_ent["thr_at"], n_ent["sym_below"], n_ent["sym_at"]) == ((1 << 20) - 2, 1 << 20, (1 << 20) - 2, 1 << 20)
    assert cen["tiles257"]["n_tiles"] == 257 and cen["tiles257"]["n_valid_last"] == 2 and cen["tiles257"]["L"] == 2
    assert [cen[f"tile_tail/{k}"]["n_valid_last"] for k in (64, 66)] == [64, 66] and cen["tile_tail/64"]["n_tiles"] == 129
    assert [cen[k]["passes"] for k in ("pass1/255", "pass2/256", "pass2/65535", "pass3/65536", "pass3/70000", "pass4")] == [1, 2, 2, 3, 3, 4]
    assert cen["many_gaps"]["listed"] == 1100 and (cen["many_gaps"]["leading"], cen["many_gaps"]["trailing"]) == (31, 32)
    assert (cen["gaps"]["leading"], cen["gaps"]["trailing"]) == (32, 31) and {31, 32} <= cen["gaps"]["between"]
    assert all(v["n_ent"] >= (1 << 20) for k, v in cen.items() if k not in ("thr_below", "sym_below"))


def test_sides_reference_on_a_hand_written_example():
    #        record:  0    1    2    3    4    5
    qid = np.array([2, 0, 2, 1, 0, 2], np.int32)
    qs = np.array([10, 30, 50, 70, 90, 110], np.int32)
    qe = qs + 10
    tid = np.array([0, 0, 3, 2, 1, 2], np.int32)              # records 1 and 5 are self overlaps: no target side
    ts = np.array([1, 3, 5, 7, 9, 12], np.int32)
    te = np.array([2, 4, 6, 8, 11, 13], np.int32)
    off, s, e = sides_reference(4, qid, qs, qe, tid, ts, te, False)
    assert off.dtype == np.int64 and off.tolist() == [0, 3, 5, 9, 10]
    assert s.tolist() == [30, 90, 1, 70, 9, 10, 50, 110, 7, 5] and e.tolist() == [40, 100, 2, 80, 11, 20, 60, 120, 8, 6]
    off, s, e = sides_reference(4, qid, qs, qe, tid, ts, te, True)
    assert off.tolist() == [0, 2, 3, 6, 6] and s.tolist() == [30, 90, 70, 10, 50, 110] and e.tolist() == [40, 100, 80, 20, 60, 120]
    off, s, e = sides_reference(3, qid[:0], qs[:0], qe[:0], tid[:0], ts[:0], te[:0], False)
    assert off.tolist() == [0, 0, 0, 0] and s.size == e.size == 0
    assert side_keys(4, qid, tid, False).tolist() == [2, 0, 2, 1, 0, 2, 0, 4, 3, 2, 1, 4]
    st, en = T.side_tags(5)
    assert st.view(np.uint32).tolist() == [0, 0x80000001, 2, 0x80000003, 4] and st[1] < 0 and len(set(en.tolist())) == 5


def test_the_comparator_fails_and_says_where():
    case = next(c for c in bucket_sort_cases("dists") if c.name == "dists/uniform/n_reads=255")
    name, n_reads, cols, sym = case
    want = sides_reference(n_reads, *cols, sym)
    assert sides_first_difference(name, n_reads, cols, sym, tuple(a.copy() for a in want), want) is None
    off, s, e = want
    n_rec = cols[0].size
    r = 100
    a = int(off[r])
    assert off[r + 1] - a >= 2

    def said(got, place, key, extra):
        with pytest.raises(AssertionError) as err:
            assert_same_sides(name, n_reads, cols, sym, got, want)
        msg = str(err.value)
        slot = int(s[place]) & 0x7FFFFFFF
        which = f"query side of record {slot}" if slot < n_rec else f"target side of record {slot - n_rec}"
        assert f"case {name}: first differing side at sorted place {place} (tile {place // PAIR_TILE}), key {key} of 255 reads" in msg, msg
        assert f"slot {slot} (tile {slot // PAIR_TILE}: the {which})" in msg and extra in msg, msg
    # two sides of one read swapped: the same multiset under every key, only the stable order tells
    s2, e2 = s.copy(), e.copy()
    s2[[a, a + 1]] = s[[a + 1, a]]; e2[[a, a + 1]] = e[[a + 1, a]]
    said((off, s2, e2), a, r, f"= slot {int(s[a + 1]) & 0x7FFFFFFF}")
    # the last side of a read moved to the read behind it: the columns are the same, one offset is not
    o2 = off.copy(); o2[r + 1] -= 1
    said((o2, s, e), int(off[r + 1]) - 1, r, f"off[{r + 1}] is {int(off[r + 1]) - 1}, want {int(off[r + 1])}")
    # one offset off by one the other way, and the count of sides with it
    o3 = off.copy(); o3[-1] += 1
    with pytest.raises(AssertionError, match=rf"case {name}: first differing side at sorted place {s.size} .*past the {s.size} sides"):
        assert_same_sides(name, n_reads, cols, sym, (o3, s, e), want)
    # a side lost, a side with another side's end
    with pytest.raises(AssertionError, match="first differing side at sorted place 7 "):
        assert_same_sides(name, n_reads, cols, sym, (off, np.delete(s, 7), np.delete(e, 7)), want)
    e4 = e.copy(); e4[5000] = e[5001]
    with pytest.raises(AssertionError, match=r"sorted place 5000 \(tile 1\)"):
        assert_same_sides(name, n_reads, cols, sym, (off, s, e4), want)


PASS_NAMES = [c.name for c in bucket_pass_cases()]


@pytest.mark.parametrize("name", PASS_NAMES)
def test_pass_cases_hold_what_they_say(name):
    case = next(c for c in bucket_pass_cases() if c.name == name)
    _, p, cols = case
    rl, qid, qs, qe, tid, ts, te = cols
    want = oracle_run(p, *cols)
    n = qid.size
    assert want["symmetric"] == int(case.symmetric)
    assert want["n_intervals"] == (n if case.symmetric else n + int((qid != tid).sum()))
    off, s, e = sides_reference(rl.size, qid, qs, qe, tid, ts, te, case.symmetric)
    assert off[-1] == want["n_intervals"] == s.size
    if case.conditions:
        assert want["rep_s"].size >= 100 and int((np.diff(want["frag_offset"]) > 1).sum()) >= 100, (want["rep_s"].size,)
    else:
        assert name in ("pass4", "many_gaps")
    last1 = (e.astype(np.int64) - 1) // p.reso + 1              # one past a side's last window: what a window record holds
    assert p.reso == (1 if name.startswith("edge16") else 50)
    if case.wide:
        assert name == "edge16_wide" and last1.max() == 65536 and int((last1 > 65535).sum()) == 1
    else:
        assert last1.max() <= 65535
    if name.startswith("edge16"):
        assert int((last1 == 65535).sum()) >= 100 and int((s // p.reso == 65534).sum()) >= 100
        assert set(rl.tolist()) == ({65534, 65535} if name == "edge16_fits" else {65534, 65535, 65536})
    if name in ("thr_at", "gaps"):
        assert np.array_equal(sides_pileup(p.reso, rl, off, s, e), want["cov"])
    if name == "self_only":
        assert np.array_equal(qid, tid)
    if name == "one_read":
        assert np.unique(qid).size == 1 and rl[qid[0]] == 60000 and np.diff(off).max() >= 1 << 15          # a deep tile
    if name == "pass4":
        assert rl.size == 1 << 24 and rl.min() == 1 and rl.max() == 50
