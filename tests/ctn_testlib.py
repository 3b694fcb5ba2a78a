"""The oracle of the containment forest and of its placement on a layout (include/raft_hip_ctn.h), and the streams its tests share.
The views and their keys are the header's formulas over the kinds that ``test_gpu_overlap_ends.want_kinds`` computes; the forest is a
sequential walk in plain Python, a read after its parent.  Nothing here runs on a device."""
import numpy as np
from test_gpu_overlap_ends import want_kinds

HAS_PARENT, PARENT_REV, ROOT_REV, UNPLACED_VIEW, ORPHAN = 1, 2, 4, 8, 16
ID_MASK = 0x7FFFFFFF
SUMMARY = ["records", "containment_views", "views_not_longer", "reads_with_parent", "orphans", "roots", "roots_with_tree", "greatest_depth",
           "largest_tree_reads", "largest_tree_bases", "launches"]
PER_READ = dict(parent=np.int32, pos=np.int32, span=np.int32, root=np.int32, root_pos=np.int32, depth=np.int32, children=np.int32, flags=np.uint8,
                tree_reads=np.int32, tree_bases=np.int64, tree_depth=np.int32)
PLACE_SUMMARY = ["n_reads", "n_unitigs", "placed", "unplaced", "unitigs_gained", "greatest_depth_permille"]
PLACE_PER_READ = dict(placed_unitig=np.int32, start=np.int64, placed_orient=np.uint8)
PLACE_PER_UNITIG = dict(placed_reads=np.int32, placed_bases=np.int64, depth_permille=np.int64)


def rounds(n_reads):
    k = 0
    while (1 << k) < max(n_reads, 2):
        k += 1
    return k


def launches(n_reads, n_rec):
    return (2 if n_rec else 0) + (3 + rounds(n_reads) if n_reads else 0)


def views(read_len, cols, strand, H, F, symmetric):
    """Every containment view of the stream as int64 columns r, c, as, ae, bs, be, rev."""
    qid, qs, qe, tid, ts, te = (np.asarray(c, np.int64) for c in cols)
    if qid.size == 0:
        return tuple(np.zeros(0, np.int64) for _ in range(7))
    n = len(read_len)
    assert ((0 <= qid) & (qid < n) & (0 <= tid) & (tid < n)).all(), "the oracle takes streams without bad ids"
    kinds = want_kinds(read_len, cols, strand, H, F)
    rev = (np.asarray(strand) != 0).astype(np.int64)
    q = kinds == 2
    t = (kinds == 3) if not symmetric else np.zeros(q.size, bool)
    cat = lambda a, b: np.concatenate([a[q], b[t]])
    return cat(qid, tid), cat(tid, qid), cat(qs, ts), cat(qe, te), cat(ts, qs), cat(te, qe), cat(rev, rev)


def oracle(read_len, cols, strand, H=1000, F=800, symmetric=False) -> dict:
    L = np.asarray(read_len, np.int64)
    n = L.size
    r, c, a_s, a_e, b_s, b_e, rev = views(L, cols, strand, H, F, symmetric)
    lr, lc = L[r], L[c]
    ok = (lc > lr) | ((lc == lr) & (c < r))
    flags = np.zeros(n, np.int64)
    flags[r[~ok]] |= UNPLACED_VIEW
    key1 = np.zeros(n, np.uint64)
    np.maximum.at(key1, r[ok], ((lc[ok] << 31) | (ID_MASK - c[ok])).astype(np.uint64))
    parent = np.where(key1 != 0, ID_MASK - (key1 & np.uint64(ID_MASK)).astype(np.int64), -1)
    named = ok & (parent[r] == c)
    span = np.minimum(a_e - a_s, b_e - b_s)
    pos = np.clip(np.where(rev != 0, b_s - (lr - a_e), b_s - a_s), 0, np.maximum(lc - lr, 0))
    key2 = np.zeros(n, np.uint64)
    np.maximum.at(key2, r[named], ((span[named] << 32) | (rev[named] << 31) | (ID_MASK - pos[named])).astype(np.uint64))
    has = parent >= 0
    assert ((key2 != 0) == has).all()
    p_pos = np.where(has, ID_MASK - (key2 & np.uint64(ID_MASK)).astype(np.int64), 0)
    p_rev = np.where(has, (key2 >> np.uint64(31)).astype(np.int64) & 1, 0)
    p_span = np.where(has, (key2 >> np.uint64(32)).astype(np.int64), 0)
    flags[has] |= HAS_PARENT
    flags[has & (p_rev != 0)] |= PARENT_REV
    flags[~has & (flags != 0)] |= ORPHAN
    # the walk, one read after the other, a read after its parent (the longer read, then the smaller id: that order is a walk's)
    root, root_pos, root_rev, depth = np.arange(n), np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    for x in sorted(range(n), key=lambda x: (-int(L[x]), x)):
        a = int(parent[x])
        if a < 0:
            continue
        assert L[a] > L[x] or (L[a] == L[x] and a < x)
        p, v, P, V = int(p_pos[x]), int(p_rev[x]), int(root_pos[a]), int(root_rev[a])
        root[x], depth[x], root_rev[x] = root[a], depth[a] + 1, v ^ V
        root_pos[x] = P + (int(L[a]) - p - int(L[x])) if V else P + p
        assert 0 <= root_pos[x] <= L[root[x]] - L[x]
    flags[root_rev != 0] |= ROOT_REV
    children = np.bincount(parent[has], minlength=n)
    below = depth > 0
    tree_reads = np.bincount(root[below], minlength=n)
    tree_bases = np.bincount(root[below], weights=L[below], minlength=n).astype(np.int64) if n else np.zeros(0, np.int64)
    tree_depth = np.zeros(n, np.int64)
    np.maximum.at(tree_depth, root[below], depth[below])
    n_rec = int(np.asarray(cols[0]).size)
    summary = dict(records=n_rec, containment_views=int(r.size), views_not_longer=int((~ok).sum()), reads_with_parent=int(has.sum()),
                   orphans=int((flags & ORPHAN != 0).sum()), roots=int((~has).sum()), roots_with_tree=int((tree_reads > 0).sum()),
                   greatest_depth=int(depth.max()) if n else 0, largest_tree_reads=int(tree_reads.max()) if n else 0,
                   largest_tree_bases=int(tree_bases.max()) if n else 0, launches=launches(n, n_rec))
    out = dict(parent=parent, pos=p_pos, span=p_span, root=root, root_pos=root_pos, depth=depth, children=children, flags=flags,
               tree_reads=tree_reads, tree_bases=tree_bases, tree_depth=tree_depth)
    return {**{k: np.asarray(v).astype(PER_READ[k]) for k, v in out.items()}, "summary": summary}


def place_oracle(read_len, forest, unitig, offset, orient, utg_length) -> dict:
    L = np.asarray(read_len, np.int64)
    n, U = L.size, len(utg_length)
    out = {k: np.zeros(n, dt) for k, dt in PLACE_PER_READ.items()}
    out["placed_unitig"][:] = -1
    reads, bases, contained = np.zeros(U, np.int64), np.zeros(U, np.int64), np.zeros(U, np.int64)
    for x in range(n):
        R = int(forest["root"][x])
        u = int(unitig[R])
        if u < 0:
            continue
        off, o, rp = int(offset[R]), int(orient[R] != 0), int(forest["root_pos"][x])
        out["placed_unitig"][x] = u
        out["start"][x] = off + (int(L[R]) - rp - int(L[x])) if o else off + rp
        out["placed_orient"][x] = o ^ (1 if forest["flags"][x] & ROOT_REV else 0)
        reads[u] += 1
        bases[u] += max(int(L[x]), 0)
        contained[u] += 1 if R != x else 0
    depth = np.array([0 if int(utg_length[u]) == 0 else int(bases[u]) * 1000 // int(utg_length[u]) for u in range(U)], np.int64)
    placed = int((out["placed_unitig"] >= 0).sum())
    summary = dict(n_reads=n, n_unitigs=U, placed=placed, unplaced=n - placed, unitigs_gained=int((contained > 0).sum()),
                   greatest_depth_permille=int(depth.max()) if U else 0)
    return {**out, "placed_reads": reads.astype(np.int32), "placed_bases": bases, "depth_permille": depth, "summary": summary}


# ---- streams
def records(rows):
    """rows of (q, qs, qe, t, ts, te, rev) -> the six columns and the strand bytes"""
    a = np.asarray(rows, np.int64).reshape(-1, 7)
    return [np.ascontiguousarray(a[:, k]).astype(np.int32) for k in range(6)], np.ascontiguousarray(a[:, 6]).astype(np.uint8)


def whole_inside(r, c, L, pos, rev, from_target=False):
    """One record that aligns read r whole with [pos, pos + len r) of read c, written from r (kind 2) or from c (kind 3)"""
    lr = int(L[r])
    return (c, pos, pos + lr, r, 0, lr, rev) if from_target else (r, 0, lr, c, pos, pos + lr, rev)


def chain(depth, strands, seed=0, shuffle=True):
    """depth + 1 reads, read k + 1 whole inside read k at a random place, on the strand strands[k]; the ids permuted.
    -> L, cols, strand"""
    rng = np.random.default_rng(seed + depth)
    n = depth + 1
    ids = rng.permutation(n) if shuffle else np.arange(n)
    L = np.zeros(n, np.int32)
    L[ids] = 40000 - 11 * np.arange(n)
    rows = []
    for k in range(depth):
        r, c = int(ids[k + 1]), int(ids[k])
        rows.append(whole_inside(r, c, L, int(rng.integers(0, 12)), int(strands[k]), from_target=bool(k & 1)))
    cols, strand = records(rows)
    return L, cols, strand


def star(n_children, seed=0, shuffle=False):
    """One parent of 30000 bases and n_children reads inside it, each by two records (one from either side)"""
    rng = np.random.default_rng(seed + n_children)
    L = np.concatenate([[30000], rng.integers(500, 9000, n_children)]).astype(np.int32)
    rows = []
    for r in range(1, n_children + 1):
        pos = int(rng.integers(0, 30000 - int(L[r]) + 1))
        rows.append(whole_inside(r, 0, L, pos, int(rng.integers(0, 2)), from_target=bool(r & 1)))
    rows = [rows[i] for i in (rng.permutation(len(rows)) if shuffle else range(len(rows)))]
    cols, strand = records(rows)
    return L, cols, strand


def reordered(cols, strand, order):
    return [np.ascontiguousarray(c[order]) for c in cols], np.ascontiguousarray(strand[order])
