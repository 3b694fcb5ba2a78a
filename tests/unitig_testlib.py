"""What the unitig tests share: a sequential walk over a table of best overlaps (the oracle of include/raft_hip_utg.h -- the
reference has no graph step), a generator of tables with chains, cycles, singletons and skipped reads by construction, and the numpy /
plain restatements of the CLI's N50, stdout line and two files."""
import numpy as np

MUTUAL, REV, SKIPPED = 2, 1, 16
SUMMARY = ("reads_in", "reads_skipped", "unitigs", "singletons", "circular", "longest_reads", "longest_length", "total_length")
PER_READ = (("unitig", np.int32), ("index", np.int32), ("offset", np.int64), ("orient", np.uint8))
PER_UNITIG = (("utg_reads", np.int32), ("utg_length", np.int64), ("utg_circular", np.uint8))


def rounds_of(n_reads):
    """ceil(log2(2 * n_reads)): the rounds of one ranking"""
    r = 0
    while (1 << r) < 2 * n_reads:
        r += 1
    return r


def first_bad_read(read_len, partner, span, flags):
    """The consistency rule, end by end: the smallest read with a violating end, or -1."""
    n = len(read_len)
    L = [max(int(x), 0) for x in read_len]
    P, S, F = np.asarray(partner).reshape(-1).tolist(), np.asarray(span).reshape(-1).tolist(), np.asarray(flags).tolist()
    for r in range(n):
        for e in range(2):
            if not (F[r] >> (2 * e)) & MUTUAL:
                continue
            p, rev = P[2 * r + e], (F[r] >> (2 * e)) & REV
            pe = e if rev else 1 - e
            ok = not F[r] & SKIPPED and 0 <= p < n and p != r
            ok = ok and not F[p] & SKIPPED and (F[p] >> (2 * pe)) & MUTUAL and ((F[p] >> (2 * pe)) & REV) == rev
            ok = ok and P[2 * p + pe] == r and S[2 * r + e] == S[2 * p + pe] and 1 <= S[2 * r + e] <= min(L[r], L[p])
            if not ok:
                return r
    return -1


def walk(read_len, partner, span, flags):
    """The unitigs of a consistent table, one read after the other: every output array of raft_hip_unitigs_* cut to U, and the summary."""
    n = len(read_len)
    L = [max(int(x), 0) for x in read_len]
    P, S, F = np.asarray(partner).reshape(-1).tolist(), np.asarray(span).reshape(-1).tolist(), np.asarray(flags).tolist()

    def mutual(r, e):
        return (F[r] >> (2 * e)) & MUTUAL

    def step(r, e):                      # leaving r through e -> the partner and the end the walk enters it at
        return P[2 * r + e], (e if (F[r] >> (2 * e)) & REV else 1 - e)

    def to_the_end(r, e):                # -> the terminal read and its free end, or None where the walk comes back to r
        cur = r
        while mutual(cur, e):
            p, e_in = step(cur, e)
            if p == r:
                return None
            seen[p] = True
            cur, e = p, 1 - e_in
        return cur, e

    seen = [False] * n
    starts = []                          # (start read, the end it is left through, circular)
    for r in range(n):
        if F[r] & SKIPPED or seen[r]:
            continue
        seen[r] = True
        a = to_the_end(r, 0)
        if a is None:                    # r is the smallest read of a cycle: every smaller one has been seen with its whole component
            starts.append((r, 1, True))
            continue
        b = to_the_end(r, 1)
        if a[0] == b[0]:
            starts.append((r, 1, False))
        else:
            t, free = a if a[0] < b[0] else b
            starts.append((t, 1 - free, False))
    starts.sort()
    unitig, index, offset, orient = [-1] * n, [-1] * n, [0] * n, [0] * n
    order, utg_off, utg_reads, utg_length, utg_circular = [], [0], [], [], []
    for u, (s, e, circular) in enumerate(starts):
        cur, off, k = s, 0, 0
        while True:
            unitig[cur], index[cur], offset[cur], orient[cur] = u, k, off, 1 - e
            order.append(cur)
            k += 1
            if not mutual(cur, e):
                length = off + L[cur]
                break
            p, e_in = step(cur, e)
            off += L[cur] - S[2 * cur + e]
            if circular and p == s:
                length = off
                break
            cur, e = p, 1 - e_in
        utg_off.append(len(order)); utg_reads.append(k); utg_length.append(length); utg_circular.append(1 if circular else 0)
    skipped = sum(1 for f in F if f & SKIPPED)
    summary = dict(reads_in=n, reads_skipped=skipped, unitigs=len(starts), singletons=sum(1 for k in utg_reads if k == 1), circular=sum(utg_circular),
                   longest_reads=max(utg_reads, default=0), longest_length=max(utg_length, default=0), total_length=sum(utg_length))
    return dict(unitig=np.array(unitig, np.int32), index=np.array(index, np.int32), offset=np.array(offset, np.int64), orient=np.array(orient, np.uint8),
                order=np.array(order, np.int32), utg_off=np.array(utg_off, np.int64), utg_reads=np.array(utg_reads, np.int32),
                utg_length=np.array(utg_length, np.int64), utg_circular=np.array(utg_circular, np.uint8), summary=summary)


def make_table(rng, n_reads, chains, skipped=0, len_range=(50, 5000), orients=None, junk=True, span_max=None):
    """A table with the given components by construction: a random permutation of the read ids is cut into ``chains`` -- (length,
    circular) pairs, in that order -- every edge on a random strand (``orients``: per chain the orientation of every read in it, instead
    of random ones), the reads behind them stand alone, ``skipped`` of those flagged SKIPPED.  Lengths and spans are chosen so that
    the rule holds (``span_max``: no overlap is longer).  ``junk``: the ends that are not mutual hold partners, spans and REV bits that nobody may look at.
    -> read_len, partner [n, 2], span [n, 2], flags"""
    assert sum(k for k, _ in chains) <= n_reads and all(k >= 1 and (k >= 2 or not c) for k, c in chains)
    perm = rng.permutation(n_reads)
    L = rng.integers(len_range[0], len_range[1] + 1, n_reads).astype(np.int64)
    partner, span, flags = np.full((n_reads, 2), -1, np.int64), np.zeros((n_reads, 2), np.int64), np.zeros(n_reads, np.int64)
    if junk and n_reads:
        partner[:] = rng.integers(-5, n_reads + 5, (n_reads, 2))
        span[:] = rng.integers(-3, len_range[1] + 3, (n_reads, 2))
        flags[:] = rng.integers(0, 2, n_reads) * 1 + rng.integers(0, 2, n_reads) * 4
    at = 0
    for c, (k, circular) in enumerate(chains):
        reads = perm[at:at + k]
        at += k
        o = rng.integers(0, 2, k) if orients is None or orients[c] is None else np.asarray(orients[c])
        for i in range(k if circular else k - 1):
            a, b, oa, ob = reads[i], reads[(i + 1) % k], o[i], o[(i + 1) % k]
            e_out, e_in = 1 - oa, ob         # '+' in the chain: entered at 5', left through 3'
            rev = 1 if e_in == e_out else 0
            s = int(rng.integers(1, min(L[a], L[b], span_max or L[a]) + 1))
            for r, e, p in ((a, e_out, b), (b, e_in, a)):
                partner[r, e], span[r, e] = p, s
                flags[r] = (flags[r] & ~(3 << (2 * e))) | ((MUTUAL | rev) << (2 * e))
    alone = perm[at:]
    flags[alone[:skipped]] |= SKIPPED
    return L.astype(np.int32), partner.astype(np.int32), span.astype(np.int32), flags.astype(np.uint8)


def n50(lengths):
    """The smallest length such that the unitigs at least that long hold half of the total (0 for none)."""
    v = sorted((int(x) for x in lengths), reverse=True)
    total, cum = sum(v), 0
    for x in v:
        cum += x
        if 2 * cum >= total:
            return x
    return 0


def stdout_line(w):
    s = w["summary"]
    return (f"INFO, unitigs(), reads = {s['reads_in']}, left out = {s['reads_skipped']}, unitigs = {s['unitigs']}, singletons = {s['singletons']}, "
            f"circular = {s['circular']}, longest = {s['longest_reads']} reads, longest length = {s['longest_length']}, "
            f"total length = {s['total_length']}, N50 = {n50(w['utg_length'])}")


def files_of(w, names, read_len):
    """-> the text of PREFIX.unitigs.tsv and of PREFIX.unitigs.layout.tsv"""
    order, off = w["order"], w["utg_off"]
    table = "".join(f"{u}\t{w['utg_reads'][u]}\t{w['utg_length'][u]}\t{w['utg_circular'][u]}\t{names[order[off[u]]]}\t{names[order[off[u + 1] - 1]]}\n"
                    for u in range(len(off) - 1))
    layout = "".join(f"{w['unitig'][r]}\t{w['index'][r]}\t{names[r]}\t{read_len[r]}\t{'-' if w['orient'][r] else '+'}\t{w['offset'][r]}\n" for r in order)
    return table, layout
