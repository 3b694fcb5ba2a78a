"""CPU: the yardstick of raft_hip_frag_overlaps_* (include/raft_hip_frag.h) -- ``want_fragments``, the header's definitions restated in
numpy -- pinned on hand-written cases with literal expected numbers, and the case lists tests/test_gpu_fragment_overlaps.py imports.

The model is deliberately not the kernel's arithmetic: no ranges, no searches, no difference arrays and no scan.  Every counted side is
compared with every row of its read (the j-th row of every read at once, j = 0, 1, ...) by the three predicates as the header writes
them, in 64-bit integers, and the partner's side with every row of the partner's read.

Which fixture supplies which class (``test_the_fixtures_show_every_class``; table = the goldens' exp_frag_*, annotation = their
exp_rep_*, both from the reference binary; symmetric = 0): on each of s150_reso1, s200_smallparams, s300_default, s300_sym_shuffled,
s300_nonsym_shuffled and s60_ultralong there are rows with frag_contained > 0 and rows with frag_contained == 0, rows with
frag_span > frag_contained, reads with all, some and no rows contained, and reads with several rows.  Untouched rows exist on
edge_reads and s60_ultralong only: the generated stream (``stream``) plants more -- rows behind the end of their read -- and the
hand-written cases show each boundary by itself.
"""
import os
import re

import numpy as np
import pytest
from raft_testlib import GOLDEN, ROOT
from test_repeat_overlaps_cases import csr, i32, union_pieces

ARRAYS = ("frag_touch", "frag_span", "frag_contained", "frag_repeat", "read_contained")
SUMMARY = ("n_records", "n_fragments", "frags_untouched", "frags_spanned", "frags_contained", "frags_contained_repeat", "reads_whole_spanned",
           "reads_any_contained", "reads_all_contained")


def _constant(path, name):
    text = open(os.path.join(ROOT, "raft_amd", "csrc", path)).read()
    return int(re.search(r"constexpr int " + name + r"\s*=\s*(\d+)\s*;", text).group(1))


def source_units():
    """The unit sizes of the record kernel and of the scan, read back from the sources: records per lane, wave, workgroup and turn of
    the grid-stride loop; slots per tile of the scan and per turn of its loop over the tiles before."""
    frag = open(os.path.join(ROOT, "raft_amd", "csrc", "frag_ovl.hpp")).read()
    # the record kernel is launched with the shared constants and has no grid function of its own
    assert '#include "record_stream.hpp"' in frag and "__launch_bounds__(kStreamThreads) void frag_side_kernel" in frag
    assert "frag_grid" not in frag
    threads, lane, blocks = (_constant("record_stream.hpp", n) for n in ("kStreamThreads", "kStreamLaneRecords", "kStreamMaxBlocks"))
    scan_threads, scan_items = _constant("device_scan.hpp", "kScanThreads"), _constant("device_scan.hpp", "kScanItems")
    return {"lane": lane, "wave": 64 * lane, "workgroup": threads * lane, "grid": blocks * threads * lane,
            "tile": scan_threads * scan_items, "segment": scan_threads * scan_threads * scan_items}


UNITS = source_units()
LANE_RECORDS, WAVE_RECORDS, WG_RECORDS, GRID_RECORDS = UNITS["lane"], UNITS["wave"], UNITS["workgroup"], UNITS["grid"]
SCAN_TILE, SCAN_SEGMENT = UNITS["tile"], UNITS["segment"]
COUNTS = (0, 1, LANE_RECORDS - 1, LANE_RECORDS, LANE_RECORDS + 1, WAVE_RECORDS - 1, WAVE_RECORDS, WAVE_RECORDS + 1, WG_RECORDS - 1, WG_RECORDS,
          WG_RECORDS + 1, GRID_RECORDS + 5)
ROW_COUNTS = (1, 2, 3, 4, 5, 63, 64, 65, 1000)
TABLE_SIZES = (0, 1, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, SCAN_SEGMENT - 1, SCAN_SEGMENT, SCAN_SEGMENT + 1)
HOT_COUNTS = (WG_RECORDS, 3 * WG_RECORDS + 1)


def test_the_units_are_what_the_case_lists_assume():
    assert UNITS == {"lane": 4, "wave": 256, "workgroup": 1024, "grid": 2048 * 1024, "tile": 2048, "segment": 256 * 2048}


def _padded(offset, values):
    """[n_reads, W] of the reads' rows, row j of read r at [r, j]; valid[r, j] says whether there is one."""
    n_reads = len(offset) - 1
    count = np.diff(offset)
    W = int(count.max()) if n_reads else 0
    out = np.zeros((max(n_reads, 1), max(W, 1)), np.int64)
    valid = np.zeros(out.shape, bool)
    for j in range(W):
        m = np.flatnonzero(count > j)
        out[m, j] = values[offset[m] + j]
        valid[m, j] = True
    return out, valid, W


def want_fragments(read_len, qid, qs, qe, tid, ts, te, symmetric, frag_offset, frag_begin, frag_end, rep_offset=None, rep_s=None, rep_e=None):
    """What Engine.fragment_overlaps returns, from the definitions of include/raft_hip_frag.h.  No annotation: frag_repeat is 0."""
    read_len, qid, qs, qe, tid, ts, te = (np.asarray(x).astype(np.int64) for x in (read_len, qid, qs, qe, tid, ts, te))
    off, fb, fe = (np.asarray(x).astype(np.int64) for x in (frag_offset, frag_begin, frag_end))
    n_reads, n_rec, n_frag = len(read_len), len(qid), len(fb)
    assert off[0] == 0 and off[-1] == n_frag and (np.diff(off) >= 0).all() and (fb >= 0).all() and (fb <= fe).all()
    FB, valid, W = _padded(off, fb)
    FE, _, _ = _padded(off, fe)
    other = qid != tid
    # the counted sides: (read, a, b) with partner (read, c, d)
    sides = [(qid[other], qs[other], qe[other], tid[other], ts[other], te[other])]
    if not symmetric:
        sides.append((tid[other], ts[other], te[other], qid[other], qs[other], qe[other]))
    r, a, b, p, c, d = (np.concatenate([s[k] for s in sides]) for k in range(6))
    keep = b > a
    r, a, b, p, c, d = (x[keep] for x in (r, a, b, p, c, d))
    whole = np.zeros(len(r), bool)
    for g in range(W):
        whole |= valid[p, g] & (FB[p, g] <= c) & (d <= FE[p, g])
    whole &= d > c
    touch, span, cont = (np.zeros(n_frag, np.int64) for _ in range(3))
    for j in range(W):
        m = np.flatnonzero(valid[r, j])
        row_b, row_e = FB[r[m], j], FE[r[m], j]
        touched = (row_e > a[m]) & (row_b < b[m])
        spanned = (row_b >= a[m]) & (row_e <= b[m]) & touched
        k = off[r[m]] + j
        touch += np.bincount(k[touched], minlength=n_frag)
        span += np.bincount(k[spanned], minlength=n_frag)
        cont += np.bincount(k[spanned & whole[m]], minlength=n_frag)
    repeat = np.zeros(n_frag, np.int64)
    if rep_offset is not None:
        rep_offset = np.asarray(rep_offset, np.int64)
        for read in np.flatnonzero(np.diff(rep_offset) > 0):
            pieces = union_pieces(zip(rep_s[rep_offset[read]:rep_offset[read + 1]], rep_e[rep_offset[read]:rep_offset[read + 1]]))
            for k in range(off[read], off[read + 1]):
                repeat[k] = sum(max(min(fe[k], e) - max(fb[k], s), 0) for s, e in pieces)
    row_read = np.repeat(np.arange(n_reads), np.diff(off))
    read_contained = np.bincount(row_read[cont > 0], minlength=n_reads)
    whole_read = np.zeros(n_reads, bool)
    whole_read[r[(a <= 0) & (b >= read_len[r])]] = True
    rows = np.diff(off)
    out = {"frag_touch": touch.astype(np.int32), "frag_span": span.astype(np.int32), "frag_contained": cont.astype(np.int32),
           "frag_repeat": repeat.astype(np.int32), "read_contained": read_contained.astype(np.int32)}
    out.update(n_records=n_rec, n_fragments=n_frag, frags_untouched=int((touch == 0).sum()), frags_spanned=int((span > 0).sum()),
               frags_contained=int((cont > 0).sum()), frags_contained_repeat=int(((cont > 0) & (repeat > 0)).sum()),
               reads_whole_spanned=int(whole_read.sum()), reads_any_contained=int((read_contained > 0).sum()),
               reads_all_contained=int(((rows > 0) & (read_contained == rows)).sum()))
    return out


def same_fragments(got, want, what):
    for k in ARRAYS:
        g = got[k].cpu().numpy() if hasattr(got[k], "is_cuda") else got[k]
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (what, k, g.dtype, g.shape, want[k].shape)
        if not np.array_equal(g, want[k]):
            i = int(np.flatnonzero(g != want[k])[0])
            raise AssertionError(f"{what}: {k}[{i}] is {g[i]}, wanted {want[k][i]} ({int((g != want[k]).sum())} differ)")
    for k in SUMMARY:
        assert got[k] == want[k], (what, k, got[k], want[k])


# ---- hand-written cases ----------------------------------------------------------------------------------------------------------------
# One table for all: read 0 has three rows with overlap zones [3500, 4000) and [6500, 7000), read 1 one row, read 2 none, read 3 an empty
# fragment between two, read 4 one row.  Rows: read 0 -> 0, 1, 2; read 1 -> 3; read 3 -> 4, 5, 6; read 4 -> 7.
HAND_LENS = [10000, 8000, 5000, 6000, 3000]
HAND_ROWS = [[(0, 4000), (3500, 7000), (6500, 10000)], [(0, 8000)], [], [(0, 3000), (3000, 3000), (3000, 6000)], [(0, 3000)]]
HAND_RUNS = [[(1000, 2000), (3000, 4500)], [], [(0, 100)], [(2900, 3100)], [(0, 3000)]]
HAND_REPEAT = [2000, 1000, 0, 0, 100, 0, 100, 3000]
_T = (1, 0, 100)                                # a partner side inside read 1's one row: whole
_Q4 = (4, 0, 3000)                              # the side that spans read 4's one row
# name -> (records, symmetric, frag_touch, frag_span, frag_contained, read_contained, reads_whole_spanned)
HAND = {
    # a side ending exactly on row 1's fb, one base before it, one base behind it
    "side_ends_on_fb": ([(0, 0, 3500) + _T, (0, 0, 3499) + _T, (0, 0, 3501) + _T], True,
                        [3, 1, 0, 0, 0, 0, 0, 0], [0] * 8, [0] * 8, [0] * 5, 0),
    # ... on row 0's fe, one base before it, one base behind it
    "side_ends_on_fe": ([(0, 0, 4000) + _T, (0, 0, 3999) + _T, (0, 0, 4001) + _T], True,
                        [3, 3, 0, 0, 0, 0, 0, 0], [2, 0, 0, 0, 0, 0, 0, 0], [2, 0, 0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0], 0),
    # a side beginning on row 1's fb and on row 0's fe, and one base either way
    "side_starts_on_fb_and_fe": ([(0, 3500, 7000) + _T, (0, 3501, 7000) + _T, (0, 3499, 7000) + _T, (0, 4000, 5000) + _T, (0, 3999, 5000) + _T,
                                  (0, 4001, 5000) + _T], True,
                                 [4, 6, 3, 0, 0, 0, 0, 0], [0, 2, 0, 0, 0, 0, 0, 0], [0, 2, 0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0], 0),
    # the partner side fills row 1 of read 0 exactly; one base over at either end it crosses a cut
    "partner_fills_a_fragment": ([_Q4 + (0, 3500, 7000), _Q4 + (0, 3500, 7001), _Q4 + (0, 3499, 7000)], True,
                                 [0, 0, 0, 0, 0, 0, 0, 3], [0, 0, 0, 0, 0, 0, 0, 3], [0, 0, 0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 1], 1),
    # the partner side inside the zone rows 0 and 1 share; reaching the next zone from row 1; one base beyond row 1's end
    "partner_in_the_overlap_zone": ([_Q4 + (0, 3600, 3900), _Q4 + (0, 6400, 7000), _Q4 + (0, 6400, 7001)], True,
                                    [0, 0, 0, 0, 0, 0, 0, 3], [0, 0, 0, 0, 0, 0, 0, 3], [0, 0, 0, 0, 0, 0, 0, 2], [0, 0, 0, 0, 1], 1),
    "self_record": ([(4, 0, 3000, 4, 0, 3000), (1, 0, 8000, 1, 0, 8000)], False, [0] * 8, [0] * 8, [0] * 8, [0] * 5, 0),
    # qe <= qs counts nothing; an empty partner side is not whole
    "empty_sides": ([(4, 1000, 1000) + _T, (4, 2000, 1000) + _T, _Q4 + (1, 50, 50), _Q4 + (1, 60, 50)], True,
                    [0, 0, 0, 0, 0, 0, 0, 2], [0, 0, 0, 0, 0, 0, 0, 2], [0] * 8, [0] * 5, 1),
    # a side on a read without rows counts for no row (but spans its read); a partner without rows is not whole
    "read_without_rows": ([(2, 0, 5000) + _T, _Q4 + (2, 0, 100)], True,
                          [0, 0, 0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 0, 0, 1], [0] * 8, [0] * 5, 2),
    # the empty fragment [3000, 3000) is touched and spanned by what has 3000 strictly inside; a partner side on it is empty
    "empty_fragment": ([(3, 0, 6000) + _T, (3, 3000, 6000) + _T, (3, 0, 3000) + _T, (3, 2999, 3001) + _T, _Q4 + (3, 3000, 3000)], True,
                       [0, 0, 0, 0, 3, 2, 3, 1], [0, 0, 0, 0, 2, 2, 2, 1], [0, 0, 0, 0, 2, 2, 2, 0], [0, 0, 0, 3, 0], 2),
    # unless symmetric the target side is counted as well, with the query side as its partner
    "both_sides_unless_symmetric": ([_Q4 + (1, 0, 8000)], False,
                                    [0, 0, 0, 1, 0, 0, 0, 1], [0, 0, 0, 1, 0, 0, 0, 1], [0, 0, 0, 1, 0, 0, 0, 1], [0, 1, 0, 0, 1], 2),
    "query_sides_when_symmetric": ([_Q4 + (1, 0, 8000)], True,
                                   [0, 0, 0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 1], 1),
}


def hand_case(name):
    """-> (the seven columns, symmetric, (frag_offset, frag_begin, frag_end), (rep_offset, rep_s, rep_e), expected dict)"""
    recs, sym, touch, span, cont, read_contained, whole = HAND[name]
    cols = [i32(*HAND_LENS)] + [i32(*[r[k] for r in recs]) for k in range(6)]
    exp = {"frag_touch": i32(*touch), "frag_span": i32(*span), "frag_contained": i32(*cont), "frag_repeat": i32(*HAND_REPEAT),
           "read_contained": i32(*read_contained), "reads_whole_spanned": whole}
    return cols, sym, csr(HAND_ROWS), csr(HAND_RUNS), exp


@pytest.mark.parametrize("name", sorted(HAND))
def test_the_model_on_hand_written_cases(name):
    cols, sym, table, rep, exp = hand_case(name)
    got = want_fragments(*cols, sym, *table, *rep)
    for k, v in exp.items():
        assert np.array_equal(got[k], v), (name, k, np.asarray(got[k]).tolist(), np.asarray(v).tolist())
    assert got["n_records"] == len(cols[1]) and got["n_fragments"] == 8
    assert got["frags_untouched"] == int((exp["frag_touch"] == 0).sum()) and got["frags_spanned"] == int((exp["frag_span"] > 0).sum())
    assert got["frags_contained"] == int((exp["frag_contained"] > 0).sum())
    assert got["frags_contained_repeat"] == int(((exp["frag_contained"] > 0) & (exp["frag_repeat"] > 0)).sum())
    assert got["reads_any_contained"] == int((exp["read_contained"] > 0).sum())
    rows = np.array([len(r) for r in HAND_ROWS])
    assert got["reads_all_contained"] == int(((rows > 0) & (exp["read_contained"] == rows)).sum())
    assert not want_fragments(*cols, sym, *table)["frag_repeat"].any()


def test_every_row_of_a_read_contained_is_counted_once():
    cols, sym, table, rep, exp = hand_case("empty_fragment")
    got = want_fragments(*cols, sym, *table, *rep)
    assert got["reads_all_contained"] == 1 and got["reads_any_contained"] == 1 and got["frags_contained_repeat"] == 2


# ---- generated tables and streams ---------------------------------------------------------------------------------------------------

def table_reads(seed=11, n_reads=53):
    """Reads with 0, 1, 2, 3 and 40 rows: rows that overlap, an empty row, rows tied on fb, a row away from both ends of its read and rows
    behind the end of their read, which no side reaches.  With repeat runs on some of them."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(3000, 30000, n_reads).astype(np.int32)
    rows, runs = [], []
    for r in range(n_reads):
        L, kind = int(lens[r]), r % 9
        if kind == 0:
            rows.append([])
        elif kind == 1:
            rows.append([(0, L)])
        elif kind == 2:
            rows.append([(100, L - 100)])
        elif kind == 3:
            rows.append([(0, L // 2 + 200), (L // 2 - 200, L)])
        elif kind == 4:
            step = L // 40
            rows.append([(k * step, min((k + 1) * step + step // 4, L)) for k in range(40)])
        elif kind == 5:
            rows.append([(0, L // 3), (L // 3, L // 3), (L // 3, L)])
        elif kind == 6:
            rows.append([(0, L), (L + 1000, L + 2000)])
        elif kind == 7:
            rows.append([(0, 1000), (0, 2000), (1500, L)])
        else:
            rows.append([(L + 500, L + 900)])
        runs.append([[], [(200, 900), (1500, 2600)], [(0, L)], [(100, 2500), (200, 1000), (2400, 2700)]][r % 4])
    return lens, rows, runs


def stream(n_rec, seed=5):
    """n_rec records over table_reads(): the query column in sorted runs of one id (within a lane, across lanes, waves and workgroups), targets
    anywhere (some on the query's own read); sides: the whole read, a row exactly, a row with either end moved by one base, the inside of
    a row, anything, nothing."""
    lens, rows, runs = table_reads()
    table = csr(rows)
    off, fb, fe = table
    n_reads = len(lens)
    rng = np.random.default_rng(seed + n_rec)
    ids = []
    while len(ids) < n_rec:
        ids += [int(rng.integers(0, n_reads))] * int(rng.integers(1, 700) if rng.random() < 0.2 else rng.integers(1, 7))
    qid = np.array(ids[:n_rec], np.int32)
    tid = rng.integers(0, n_reads, n_rec).astype(np.int32)
    tid = np.where(rng.random(n_rec) < 0.03, qid, tid).astype(np.int32)
    count = np.diff(off)

    def sides(rid):
        L = lens[rid].astype(np.int64)
        k = off[rid] + (rng.random(n_rec) * count[rid]).astype(np.int64)
        has = count[rid] > 0
        k = np.where(has, k, 0)
        has &= fb[k] <= L                                                # (a row behind the end of its read is never aimed at)
        rb = np.where(has, fb[k] if len(fb) else 0, 0).astype(np.int64)
        re_ = np.where(has, fe[k] if len(fe) else 0, L).astype(np.int64)
        a = (rng.random(n_rec) * L).astype(np.int64)
        b = a + (rng.random(n_rec) * (L - a)).astype(np.int64)
        kind = rng.integers(0, 9, n_rec)
        a = np.where(kind == 0, 0, a); b = np.where(kind == 0, L, b)
        for code, da, db in ((1, 0, 0), (2, -1, 0), (3, 1, 0), (4, 0, 1), (5, 0, -1)):
            a = np.where(kind == code, rb + da, a); b = np.where(kind == code, re_ + db, b)
        quarter = (re_ - rb) // 4
        a = np.where(kind == 6, rb + quarter, a); b = np.where(kind == 6, re_ - quarter, b)
        b = np.where(kind == 7, a - rng.integers(0, 2, n_rec), b)
        return a.astype(np.int32), b.astype(np.int32)

    qs, qe = sides(qid)
    ts, te = sides(tid)
    return [lens, qid, qs, qe, tid, ts, te], table, csr(runs)


def one_read(n_rows):
    """Read 0 with n_rows rows of 120 bases every 100 (neighbours share 20), read 1 with one row; sides of read 0 laid on every row
    boundary and one base either way, from every row to itself and to the next; half of the partner sides cross read 1's row."""
    rows = [[(j * 100, j * 100 + 120) for j in range(n_rows)], [(0, 5000)]]
    L = n_rows * 100 + 20
    recs = []
    for j in range(n_rows):
        for m in (j, min(j + 1, n_rows - 1)):
            for da in (-1, 0, 1):
                for db in (-1, 0, 1):
                    recs.append((0, j * 100 + da, m * 100 + 120 + db, 1, 100, 4000 if (j + da + db) % 2 else 5001))
    recs.append((0, 0, L, 1, 0, 5000))
    cols = [i32(L, 5000)] + [i32(*[r[k] for r in recs]) for k in range(6)]
    return cols, csr(rows), csr([sorted([(50, 170), (L - 100, L - 10)]), []])               # (rep_s ascends within a read: what the annotation promises)


def hot_read(n_rec):
    """Every record on reads 0 and 1 (three rows and one): every side of a workgroup, and of several, lands on the same few slots."""
    rows = [[(0, 4000), (3500, 7000), (6500, 10000)], [(0, 8000)]]
    rng = np.random.default_rng(n_rec)
    edges = np.array([0, 3500, 4000, 6500, 7000, 10000])
    a = edges[rng.integers(0, 5, n_rec)] + rng.integers(-1, 2, n_rec)
    b = np.maximum(a, edges[rng.integers(1, 6, n_rec)] + rng.integers(-1, 2, n_rec))
    ts = rng.integers(0, 4000, n_rec)
    te = ts + rng.integers(0, 4100, n_rec)
    row = rng.random(n_rec) < 0.1                                          # (read 1's row itself, now and then)
    ts, te = np.where(row, 0, ts), np.where(row, 8000, te)
    cols = [i32(10000, 8000), np.zeros(n_rec, np.int32), a.astype(np.int32), b.astype(np.int32), np.ones(n_rec, np.int32), ts.astype(np.int32),
            te.astype(np.int32)]
    return cols, csr(rows)


def big_table(n_frag, n_rec=600):
    """n_frag rows over reads of 1, 2 and 3 rows in turn (no read: n_frag = 0 has one read without rows); records on the reads around every
    tile boundary of the scan, on the first and the last reads, and anywhere."""
    count, total = [], 0
    while total < n_frag:
        count.append(min(len(count) % 3 + 1, n_frag - total))
        total += count[-1]
    count = np.array(count or [0], np.int64)
    n_reads = len(count)
    off = np.zeros(n_reads + 1, np.int64)
    off[1:] = np.cumsum(count)
    j = np.arange(n_frag) - np.repeat(off[:-1], count)                # row within its read
    fb, fe = (j * 1000).astype(np.int32), (j * 1000 + 1200).astype(np.int32)
    lens = (count * 1000 + 200).astype(np.int32)
    rng = np.random.default_rng(n_frag)
    row_read = np.repeat(np.arange(n_reads), count)
    near = [row_read[k] for t in range(SCAN_TILE, n_frag + 1, SCAN_TILE) for k in (t - 2, t - 1, t, t + 1) if 0 <= k < n_frag]
    pool = np.array(sorted(set(near + [0, n_reads - 1, max(n_reads - 2, 0)])), np.int64)
    pick = lambda: np.where(rng.random(n_rec) < 0.7, pool[rng.integers(0, len(pool), n_rec)], rng.integers(0, n_reads, n_rec))
    qid, tid = np.sort(pick()).astype(np.int32), pick().astype(np.int32)
    if n_rec:
        qid[0], qid[-1] = 0, n_reads - 1                                  # (the first and the last row are touched whatever was drawn)
        tid[0], tid[-1] = n_reads - 1, 0

    def sides(rid):
        a = rng.integers(0, 3, n_rec) * 1000 + rng.integers(-1, 2, n_rec)
        b = a + rng.integers(1, 4, n_rec) * 1000 + 200 + rng.integers(-1, 2, n_rec)
        whole = rng.random(n_rec) < 0.3
        whole[:1] = whole[-1:] = True
        return np.where(whole, 0, a).astype(np.int32), np.where(whole, lens[rid], b).astype(np.int32)

    qs, qe = sides(qid)
    ts, te = sides(tid)
    return [lens, qid, qs, qe, tid, ts, te], (off, fb, fe)


GOLDENS = ("s150_reso1", "s200_smallparams", "s300_default", "s300_sym_shuffled", "s300_nonsym_shuffled", "s60_ultralong")


def golden_case(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cols = [z[k] for k in ("read_len", "qid", "qs", "qe", "tid", "ts", "te")]
    return (cols, (z["exp_frag_offset"].astype(np.int64), z["exp_frag_begin"], z["exp_frag_end"]),
            (z["exp_rep_offset"].astype(np.int64), z["exp_rep_s"], z["exp_rep_e"]))


def classes(w, table):
    """The classes a set of results shows: what the fixture census asserts on."""
    rows = np.diff(table[0])
    c = w["frag_contained"] > 0
    rc = w["read_contained"]
    return {"contained": bool(c.any()), "not contained": bool((~c).any()), "spanned beyond contained": bool((w["frag_span"] > w["frag_contained"]).any()),
            "reads all contained": bool(((rows > 0) & (rc == rows)).any()), "reads some contained": bool(((rc > 0) & (rc < rows)).any()),
            "reads none contained": bool(((rows > 0) & (rc == 0)).any()), "reads with several rows": bool((rows > 1).any()),
            "untouched": bool((w["frag_touch"] == 0).any()), "contained with repeat": bool((c & (w["frag_repeat"] > 0)).any())}


@pytest.mark.parametrize("name", GOLDENS)
def test_the_fixtures_show_every_class(name):
    cols, table, rep = golden_case(name)
    seen = classes(want_fragments(*cols, False, *table, *rep), table)
    empty = [k for k, v in seen.items() if not v and k != "untouched"]
    assert not empty, (name, empty)


def test_untouched_rows_come_from_the_edge_fixture_and_the_generated_stream():
    cols, table, rep = golden_case("edge_reads")
    assert classes(want_fragments(*cols, False, *table, *rep), table)["untouched"]
    cols, table, rep = stream(1023)
    w = want_fragments(*cols, False, *table, *rep)
    seen = classes(w, table)
    assert all(seen.values()), seen
    assert w["frags_untouched"] >= 5 and (cols[1] == cols[4]).any() and (cols[3] <= cols[2]).any()


def test_the_generated_tables_are_what_the_cases_need():
    lens, rows, runs = table_reads()
    assert {0, 1, 2, 3, 40} <= {len(r) for r in rows}
    for r in rows:
        assert [b for b, _ in r] == sorted(b for b, _ in r) and [e for _, e in r] == sorted(e for _, e in r) and all(0 <= b <= e for b, e in r)
    assert any(b == e for r in rows for b, e in r) and any(len(r) > 1 and r[0][0] == r[1][0] for r in rows)
    assert any(r and r[-1][0] > L for r, L in zip(rows, lens))
    for n in (0, 1, SCAN_TILE + 1):
        cols, (off, fb, fe) = big_table(n)
        assert off[-1] == n == len(fb) and (np.diff(off) >= (1 if n else 0)).all() and cols[1].max() == len(cols[0]) - 1
    cols, table, _ = one_read(5)
    w = want_fragments(*cols, False, *table)
    assert w["frag_span"].min() > 0 and (w["frag_span"] > w["frag_contained"]).all() and w["frag_contained"][:-1].min() > 0      # (the last row is read 1's)
    cols, table = hot_read(WG_RECORDS)
    w = want_fragments(*cols, False, *table)
    assert w["frag_touch"].min() > 100 and w["frag_contained"].min() > 0
