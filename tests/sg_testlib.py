"""The oracle of the string graph (include/raft_hip_sg.h) and the streams its tests share: the rule in plain Python and numpy over the
kinds that ``test_gpu_overlap_ends.want_kinds`` computes -- the arcs of the views, one per (u, w) by the key, adjacency as a dictionary,
the reduction by brute force over every (arc, via) pair of a row -- and a layout generator: reads placed on a line or a circle with
random strands and exact coordinates.  Nothing here runs on a device."""
import numpy as np
from test_gpu_overlap_ends import VIEW, want_kinds

SUMMARY = ["records", "dovetail_views", "views_left_out", "arcs", "duplicate_arcs", "unpaired_arcs", "reducible_arcs", "edges", "removed_edges",
           "kept_edges", "ends_with_arc", "ends_kept_one", "ends_kept_more", "ends_mutual", "ends_dead", "reads_flagged", "longest_row"]
PER_END, TABLE = ("arcs", "kept"), ("partner", "span", "flags")
EDGE_COLUMNS = ("edge_u", "edge_w", "edge_span", "edge_ext", "edge_back", "edge_flags")
RED_U, RED_W, UNPAIRED = 1, 2, 4
BEST_REV5, BEST_MUTUAL5, BEST_SKIPPED = 1, 2, 16


def view_arcs(read_len, cols, strand, H, F, symmetric, skip):
    """-> the arcs of the views as an int64 array [items, 5] (u, w, ext, back, span), and the dovetail views left out"""
    L = np.asarray(read_len, np.int64)
    if len(cols[0]) == 0:
        return np.zeros((0, 5), np.int64), 0
    qid, qs, qe, tid, ts, te = (np.asarray(c, np.int64) for c in cols)
    assert ((0 <= qid) & (qid < L.size) & (0 <= tid) & (tid < L.size)).all(), "the oracle takes streams without bad ids"
    rev = np.asarray(strand) != 0
    kinds = want_kinds(L, cols, strand, H, F).astype(np.int64)
    flagged = np.zeros(L.size, bool) if skip is None else np.asarray(skip) != 0
    out, left = [], 0
    views = [(kinds, qid, qs, qe, tid, ts, te)]
    if not symmetric:
        views.append((VIEW[rev.astype(int), kinds].astype(np.int64), tid, ts, te, qid, qs, qe))
    for kind, me, ms, me_end, other, os_, oe in views:
        lm, lo = L[me], L[other]
        q5, q3 = ms, lm - me_end
        t5, t3 = np.where(rev, lo - oe, os_), np.where(rev, os_, lo - oe)
        dovetail = (kind == 4) | (kind == 5)
        out_side = flagged[me] | flagged[other]
        left += int((dovetail & out_side).sum())
        m = dovetail & ~out_side
        E = np.where(kind == 4, 1, 0)
        Ep = np.where(rev, E, 1 - E)
        ext = np.where(E == 1, t3 - q3, t5 - q5)
        back = np.where(E == 1, q5 - t5, q3 - t3)
        span = np.minimum(me_end - ms, oe - os_)
        a = np.stack([2 * me + E, 2 * other + Ep, ext, back, span], axis=1)[m]
        assert (a[:, 2] >= 1).all() and (a[:, 3] >= 1).all()
        out.append(a)
    return np.concatenate(out), left


def choose(items):
    """One arc per (u, w): the greatest key (span, -ext_lo, -ext_hi) -> {(u, w): (ext, back, span)}"""
    chosen = {}
    for u, w, ext, back, span in items.tolist():
        lo, hi = (ext, back) if (u >> 1) < (w >> 1) else (back, ext)
        key = (span, -lo, -hi)
        old = chosen.get((u, w))
        if old is None or key > old[0]:
            chosen[(u, w)] = (key, (ext, back, span))
    return {k: v[1] for k, v in chosen.items()}


def oracle(read_len, cols, strand, H=1000, F=800, fuzz=1000, symmetric=False, skip=None, emit_removed=False) -> dict:
    L = np.asarray(read_len, np.int64)
    n = L.size
    items, left_out = view_arcs(L, cols, strand, H, F, symmetric, skip)
    arc = choose(items)
    rows = {}
    for (u, w), (ext, _, _) in arc.items():
        rows.setdefault(u, {})[w] = ext
    # brute force: every arc against every other arc of its row
    red = set()
    for u, row in rows.items():
        for w, ext_uw in row.items():
            for v, ext_uv in row.items():
                if v == w or not ext_uv < ext_uw:
                    continue
                ext_vw = rows.get(v ^ 1, {}).get(w)
                if ext_vw is not None and abs(ext_uv + ext_vw - ext_uw) <= fuzz:
                    red.add((u, w))
                    break
    survives = {(u, w) for (u, w) in arc if (u, w) not in red and (w, u) not in red}
    n_arcs, kept = np.zeros(2 * n, np.int32), np.zeros(2 * n, np.int32)
    for (u, w) in arc:
        n_arcs[u] += 1
        kept[u] += (u, w) in survives
    sole = {u: w for (u, w) in survives if kept[u] == 1}
    flagged = np.zeros(n, bool) if skip is None else np.asarray(skip) != 0
    partner, span, flags = np.full(2 * n, -1, np.int32), np.zeros(2 * n, np.int32), np.where(flagged, BEST_SKIPPED, 0).astype(np.uint8)
    mutual = 0
    for u, w in sole.items():
        if sole.get(w) == u and (w, u) in arc and arc[(w, u)][2] == arc[(u, w)][2]:
            partner[u], span[u] = w >> 1, arc[(u, w)][2]
            flags[u >> 1] |= ((BEST_REV5 if (w & 1) == (u & 1) else 0) | BEST_MUTUAL5) << (2 * (u & 1))
            mutual += 1
    edges = []
    n_edges = n_kept_edges = unpaired = 0
    for (u, w) in sorted(arc):
        twin = (w, u) in arc
        unpaired += not twin
        if twin and not (u >> 1) < (w >> 1):
            continue
        n_edges += 1
        n_kept_edges += (u, w) in survives
        if emit_removed or (u, w) in survives:
            ext, back, sp = arc[(u, w)]
            edges.append((u, w, sp, ext, back, (RED_U if (u, w) in red else 0) | (RED_W if (w, u) in red else 0) | (0 if twin else UNPAIRED)))
    e = np.array(edges, np.int64).reshape(-1, 6)
    ends_flagged = np.repeat(flagged, 2)
    summary = dict(records=int(len(cols[0])), dovetail_views=int(len(items)), views_left_out=left_out, arcs=len(arc), duplicate_arcs=int(len(items)) - len(arc),
                   unpaired_arcs=int(unpaired), reducible_arcs=len(red), edges=n_edges, removed_edges=n_edges - n_kept_edges, kept_edges=n_kept_edges,
                   ends_with_arc=int((n_arcs > 0).sum()), ends_kept_one=int((kept == 1).sum()), ends_kept_more=int((kept >= 2).sum()), ends_mutual=mutual,
                   ends_dead=int(((kept == 0) & ~ends_flagged).sum()), reads_flagged=int(flagged.sum()), longest_row=int(n_arcs.max()) if n else 0)
    res = {"arcs": n_arcs.reshape(n, 2), "kept": kept.reshape(n, 2), "partner": partner.reshape(n, 2), "span": span.reshape(n, 2), "flags": flags,
           "n_out": len(edges), "summary": summary, "reducible": red, "chosen": arc}
    for k, name in enumerate(EDGE_COLUMNS):
        res[name] = e[:, k].astype(np.uint8 if name == "edge_flags" else np.int32)
    return res


def contained(read_len, cols, strand, H=1000, F=800):
    """The skip bytes the command line builds: the reads some record shows as contained (overlap_ends' status `contained`)."""
    L = np.asarray(read_len, np.int64)
    skip = np.zeros(L.size, np.uint8)
    if len(cols[0]):
        kinds = want_kinds(L, cols, strand, H, F)
        skip[np.asarray(cols[0])[kinds == 2]] = 1
        skip[np.asarray(cols[3])[kinds == 3]] = 1
    return skip


def layout(rng, n, *, circular=False, step=(1500, 2500), length=(9000, 11000), min_overlap=500, both=False, shuffle_ids=True, strands=True):
    """n reads placed on a line (or a circle) at random steps with random strands; one record, with exact coordinates, per pair of
    reads that share ``min_overlap`` bases or more -- seen from either read at random, or with ``both`` from both (a mirrored stream).
    -> read_len, the six columns, strand, and ``slot``: the read id at each place of the layout."""
    L_slot = rng.integers(length[0], length[1] + 1, n).astype(np.int64)
    pos = np.cumsum(rng.integers(step[0], step[1] + 1, n)).astype(np.int64)
    circumference = int(pos[-1] + rng.integers(step[0], step[1] + 1) - pos[0]) if circular else None
    orient = rng.integers(0, 2, n) if strands else np.zeros(n, np.int64)
    slot = rng.permutation(n) if shuffle_ids else np.arange(n)
    rows = []
    for i in range(n):
        for j in range(n):
            if i == j:
                continue
            d = int(pos[j] - pos[i])
            if circular:
                d %= circumference
            if d < 0 or (d == 0 and j < i):
                continue
            end = min(int(L_slot[i]), d + int(L_slot[j]))
            if end - d < min_overlap:
                continue
            a, b = (d, end), (0, end - d)                   # on read i and on read j, both as laid out
            if orient[i]:
                a = (int(L_slot[i]) - a[1], int(L_slot[i]) - a[0])
            if orient[j]:
                b = (int(L_slot[j]) - b[1], int(L_slot[j]) - b[0])
            rev = int(orient[i] != orient[j])
            first = (slot[i], a[0], a[1], slot[j], b[0], b[1], rev)
            second = (slot[j], b[0], b[1], slot[i], a[0], a[1], rev)
            if both:
                rows += [first, second]
            else:
                rows.append(first if rng.random() < 0.5 else second)
    rows = np.array(rows, np.int64).reshape(-1, 7)
    rows = rows[np.argsort(rows[:, 0], kind="stable")]
    read_len = np.zeros(n, np.int32)
    read_len[slot] = L_slot
    cols = [np.ascontiguousarray(rows[:, k].astype(np.int32)) for k in range(6)]
    return read_len, cols, np.ascontiguousarray(rows[:, 6].astype(np.uint8)), slot


def reordered(cols, strand, order):
    return [np.ascontiguousarray(c[order]) for c in cols], np.ascontiguousarray(strand[order])


def stream_of(rows):
    """Rows (qid, qs, qe, tid, ts, te, rev) -> the six columns and strand"""
    rows = np.array(rows, np.int64).reshape(-1, 7)
    return [np.ascontiguousarray(rows[:, k].astype(np.int32)) for k in range(6)], np.ascontiguousarray(rows[:, 6].astype(np.uint8))


def forward_rows(pos, length, pairs):
    """Reads on one strand at places ``pos`` with lengths ``length``: one record per pair (i, j), exact -> rows for ``stream_of``"""
    rows = []
    for i, j in pairs:
        a, b = (i, j) if pos[i] <= pos[j] else (j, i)
        d = pos[b] - pos[a]
        end = min(length[a], d + length[b])
        assert end > d, (i, j)
        first, second = (a, d, end, b, 0, end - d, 0), (b, 0, end - d, a, d, end, 0)
        rows.append(first if a == i else second)
    return rows
