"""The oracle of the connected components (include/raft_hip_cc.h) and the streams its tests share: a sequential union-find in plain
Python over the kinds that ``test_gpu_overlap_ends.want_kinds`` computes, component ids made dense by smallest member.  Nothing here
runs on a device."""
import numpy as np
from test_gpu_overlap_ends import want_kinds

KINDS_PROPER, KINDS_ALL = 60, 62
SUMMARY = ["n_reads", "n_records", "edge_records", "components", "singletons", "largest_reads", "largest_bases", "total_bases",
           "reads_in_largest_permille"]
PER_READ, PER_COMPONENT = ("component", "degree"), ("comp_first", "comp_reads", "comp_bases", "comp_sides")


def edge_mask(read_len, cols, strand, H, F, kind_mask):
    """Which records are edges: both ids are reads, and the kind as the query sees it is in the mask."""
    n_reads = len(read_len)
    qid, tid = np.asarray(cols[0], np.int64), np.asarray(cols[3], np.int64)
    if qid.size == 0:
        return np.zeros(0, bool)
    assert ((0 <= qid) & (qid < n_reads) & (0 <= tid) & (tid < n_reads)).all(), "the oracle takes streams without bad ids"
    kinds = want_kinds(read_len, cols, strand, H, F).astype(np.int64)
    return ((int(kind_mask) >> kinds) & 1) != 0


def oracle(read_len, cols, strand, H=1000, F=800, kind_mask=KINDS_PROPER, symmetric=False) -> dict:
    L = np.asarray(read_len, np.int64)
    n = L.size
    qid, tid = np.asarray(cols[0], np.int64), np.asarray(cols[3], np.int64)
    edge = edge_mask(L, cols, strand, H, F, kind_mask)
    q, t = qid[edge], tid[edge]
    degree = np.bincount(q, minlength=n)
    if not symmetric:
        degree = degree + np.bincount(t, minlength=n)
    # the union-find proper, one edge after the other (a pair once: duplicates and mirrors join nothing new)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    keys = np.unique(np.minimum(q, t) * max(n, 1) + np.maximum(q, t))
    for a, b in zip((keys // max(n, 1)).tolist(), (keys % max(n, 1)).tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    root = np.fromiter((find(x) for x in range(n)), np.int64, n)
    # dense ids in the order of each component's smallest read: the root is it (the smaller root always stays one)
    first = np.flatnonzero(root == np.arange(n))
    dense = np.zeros(n, np.int64)
    dense[first] = np.arange(first.size)
    component = dense[root]
    lens = np.maximum(L, 0)
    C = first.size
    comp_reads = np.bincount(component, minlength=C)
    comp_bases = np.bincount(component, weights=lens, minlength=C).astype(np.int64) if n else np.zeros(0, np.int64)
    comp_sides = np.bincount(component, weights=degree, minlength=C).astype(np.int64) if n else np.zeros(0, np.int64)
    largest = int(comp_reads.max()) if C else 0
    summary = dict(n_reads=n, n_records=int(qid.size), edge_records=int(edge.sum()), components=C, singletons=int((comp_reads == 1).sum()),
                   largest_reads=largest, largest_bases=int(comp_bases.max()) if C else 0, total_bases=int(lens.sum()),
                   reads_in_largest_permille=largest * 1000 // n if n else 0)
    return {"component": component.astype(np.int32), "degree": degree.astype(np.int32), "comp_first": first.astype(np.int32),
            "comp_reads": comp_reads.astype(np.int32), "comp_bases": comp_bases, "comp_sides": comp_sides, "summary": summary}


def edge_stream(n_reads, pairs, length=1000):
    """Reads of one length and one record per pair (q, t), both reads aligned whole: a containment whichever way round (kind 2 or 3
    by the ids), so an edge under PROPER and ALL; q == t gives a self record."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    n = len(pairs)
    L = np.full(n_reads, length, np.int32)
    zero, full = np.zeros(n, np.int32), np.full(n, length, np.int32)
    cols = [pairs[:, 0].astype(np.int32), zero, full, pairs[:, 1].astype(np.int32), zero.copy(), full.copy()]
    return L, cols, np.zeros(n, np.uint8)


def reordered(cols, strand, order):
    return [np.ascontiguousarray(c[order]) for c in cols], np.ascontiguousarray(strand[order])
