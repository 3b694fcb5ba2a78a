"""The oracle of the lift tests: the rule of include/raft_hip_lift.h by brute force over all row pairs, in plain Python integers --
no binary search, no fast path --, the mirror of a stream, and the tables and streams the tests share."""
import numpy as np

COLUMNS = ("qfrag", "qs", "qe", "tfrag", "ts", "te", "rev", "src")
SUMMARY = ("n_records", "n_out", "records_none", "records_cut", "pairs_dropped", "most_per_record")


def ceil_div(x, y):
    return -((-x) // y)


def lift_record(off, fb, fe, rec, min_len=1):
    """rec = (qid, qs, qe, tid, ts, te, rev) -> (outputs as (qfrag, qs, qe, tfrag, ts, te) tuples in the rule's order, dropped pairs)."""
    qid, qs, qe, tid, ts, te, rev = (int(x) for x in rec)
    if qid == tid or qe <= qs or te <= ts:
        return [], 0
    swap = tid < qid
    (a, as_, ae), (b, bs, be) = ((tid, ts, te), (qid, qs, qe)) if swap else ((qid, qs, qe), (tid, ts, te))
    LA, LB = ae - as_, be - bs
    out, dropped = [], 0
    for i in range(int(off[a]), int(off[a + 1])):
        fbi, fei = int(fb[i]), int(fe[i])
        if not (fei > as_ and fbi < ae):
            continue
        for j in range(int(off[b]), int(off[b + 1])):
            fbj, fej = int(fb[j]), int(fe[j])
            if not (fej > bs and fbj < be):
                continue
            ua, ub = max(0, fbi - as_), min(LA, fei - as_)
            if rev:
                va, vb = max(0, be - fej), min(LB, be - fbj)
            else:
                va, vb = max(0, fbj - bs), min(LB, fej - bs)
            u1 = max(ua, ceil_div(va * LA, LB))
            u2 = min(ub, ceil_div((vb + 1) * LA, LB) - 1)
            if u2 - u1 < min_len:
                dropped += 1
                continue
            v1, v2 = u1 * LB // LA, u2 * LB // LA
            if v2 - v1 < min_len:
                dropped += 1
                continue
            assert va <= v1 <= v2 <= vb and ua <= u1 <= u2 <= ub
            sa = (i, as_ + u1 - fbi, as_ + u2 - fbi)
            sb = (j, be - v2 - fbj, be - v1 - fbj) if rev else (j, bs + v1 - fbj, bs + v2 - fbj)
            out.append(sb + sa if swap else sa + sb)
    return out, dropped


def lift(off, fb, fe, cols, strand, min_len=1):
    """The whole stream -> dict of the eight columns and the summary's counts."""
    rows = [[] for _ in range(8)]
    none = cut = dropped = most = 0
    n = len(cols[0])
    for r in range(n):
        rev = 1 if strand[r] else 0
        out, d = lift_record(off, fb, fe, [c[r] for c in cols] + [rev], min_len)
        dropped += d
        none += not out
        cut += len(out) > 1
        most = max(most, len(out))
        for o in out:
            for k in range(6):
                rows[k].append(o[k])
            rows[6].append(rev)
            rows[7].append(r)
    res = {name: np.asarray(rows[k], np.uint8 if name == "rev" else np.int32) for k, name in enumerate(COLUMNS)}
    res.update(n_records=n, n_out=len(rows[0]), records_none=int(none), records_cut=int(cut), pairs_dropped=dropped, most_per_record=most)
    return res


def mirror(cols, strand):
    """Every record with its sides exchanged."""
    qid, qs, qe, tid, ts, te = cols
    return [tid, ts, te, qid, qs, qe], strand


def as_multiset(res, mirrored=False):
    """The outputs as a sorted list of tuples (without src); mirrored: sides exchanged first."""
    c = [res[k].tolist() for k in COLUMNS[:7]]
    if mirrored:
        c = c[3:6] + c[0:3] + c[6:]
    return sorted(zip(*c))


def make_table(rng, n_reads, rows_choice=(0, 1, 2, 3, 40), overlaps=(0, 10, 500), base_len=1500):
    """A table that mixes reads with the given row counts; neighbouring rows of a read overlap by one of ``overlaps`` bases.
    -> read_len, frag_offset (int64), frag_begin, frag_end (int32)"""
    off, fb, fe, length = [0], [], [], []
    for r in range(n_reads):
        k = int(rows_choice[r % len(rows_choice)]) if r < 2 * len(rows_choice) else int(rng.choice(rows_choice))
        pos = int(rng.integers(0, 50))
        for _ in range(k):
            size = int(rng.integers(base_len // 2, base_len)) + 600
            fb.append(pos)
            fe.append(pos + size)
            pos = pos + size - int(rng.choice(overlaps))
        length.append((fe[-1] if k else 0) + int(rng.integers(0, 300)) + 1000)
        off.append(len(fb))
    return np.asarray(length, np.int32), np.asarray(off, np.int64), np.asarray(fb, np.int32), np.asarray(fe, np.int32)


def make_stream(rng, read_len, n_rec, rev=None, self_share=0.02):
    """n_rec records between random reads, sides anywhere inside (and a little outside) the reads.  -> six int32 columns, strand uint8"""
    n_reads = len(read_len)
    qid = rng.integers(0, n_reads, n_rec)
    tid = rng.integers(0, n_reads, n_rec)
    same = rng.random(n_rec) < self_share
    tid = np.where(same, qid, tid)

    def side(ids):
        ln = read_len[ids].astype(np.int64)
        s = (rng.random(n_rec) * ln).astype(np.int64) - rng.integers(0, 3, n_rec) * 20
        e = s + 1 + (rng.random(n_rec) ** 2 * (ln + 100)).astype(np.int64)
        empty = rng.random(n_rec) < 0.01
        return s, np.where(empty, s, e)
    qs, qe = side(qid)
    ts, te = side(tid)
    strand = (rng.integers(0, 2, n_rec) if rev is None else np.full(n_rec, rev)).astype(np.uint8)
    return [np.ascontiguousarray(c, np.int32) for c in (qid, qs, qe, tid, ts, te)], strand


def identity_table(read_len):
    """One row [0, len) per read: every in-range record lifts to itself."""
    n = len(read_len)
    return np.arange(n + 1, dtype=np.int64), np.zeros(n, np.int32), np.asarray(read_len, np.int32)
