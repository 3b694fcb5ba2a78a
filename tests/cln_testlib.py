"""The rule of include/raft_hip_cln.h in plain Python -- dictionaries and a chain walk, nothing from the device -- and builders of the
layouts the graph_clean tests use.  ``clean`` returns what ``Engine.graph_clean`` returns (but for the times), or
``{"error_index": i}`` for a list with a bad edge."""
import numpy as np

WEAK_U, WEAK_W, TIP = 1, 2, 4
REV5, MUTUAL5, SKIPPED = 1, 2, 16
# the arrays of a result, in the order of the entry point's outputs, and the fields of raft_hip_cln_summary
ARRAYS = ("edge_state", "edge_round", "read_state", "read_round", "arcs", "weak", "kept", "partner", "span", "flags")
SUMMARY = ["reads", "reads_flagged", "edges", "weak_arcs", "weak_edges", "rounds_run", "converged", "tips", "tip_reads", "tip_bases", "tip_edges",
           "candidates_kept", "isolated_short", "kept_edges", "ends_kept_one", "ends_kept_more", "ends_mutual", "ends_dead", "longest_row"]


def clean(read_len, edge_u, edge_w, edge_span, skip=None, W=500, T=4, R=3):
    n, ne = len(read_len), len(edge_u)
    length = [max(int(x), 0) for x in read_len]
    flagged = [bool(skip[r]) if skip is not None else False for r in range(n)]
    eu, ew, es = [int(x) for x in edge_u], [int(x) for x in edge_w], [int(x) for x in edge_span]
    seen = set()
    for e in range(ne):
        u, w, s = eu[e], ew[e], es[e]
        ok = 0 <= u < 2 * n and 0 <= w < 2 * n and u >> 1 != w >> 1
        ok = ok and not flagged[u >> 1] and not flagged[w >> 1] and 1 <= s <= min(length[u >> 1], length[w >> 1])
        if not ok or frozenset((u, w)) in seen:
            return {"error_index": e}
        seen.add(frozenset((u, w)))
    rows = {}                                    # node -> [(to, edge)]
    for e in range(ne):
        rows.setdefault(eu[e], []).append((ew[e], e))
        rows.setdefault(ew[e], []).append((eu[e], e))
    best = {u: max(es[e] for _, e in row) for u, row in rows.items()}
    edge_state, edge_round = [0] * ne, [0] * ne
    for e in range(ne):
        edge_state[e] = (WEAK_U if es[e] * 1000 < W * best[eu[e]] else 0) | (WEAK_W if es[e] * 1000 < W * best[ew[e]] else 0)
    read_state, read_round = [2 if f else 0 for f in flagged], [0] * n
    arcs = [len(rows.get(u, ())) for u in range(2 * n)]
    weak = [sum(1 for _, e in rows.get(u, ()) if edge_state[e]) for u in range(2 * n)]

    def live_rows():
        return {u: [(w, e) for w, e in row if edge_state[e] == 0] for u, row in rows.items()}

    def chains(live):
        """read -> its chain's record (one dict per chain, shared by its reads)"""
        deg = lambda u: len(live.get(u, ()))
        joined = lambda u: deg(u) == 1 and deg(live[u][0][0]) == 1
        of = {}
        for r in range(n):
            if read_state[r] != 0 or r in of:
                continue
            cur, end, circular = r, 0, False     # to a terminal end, leaving through end 0
            while joined(2 * cur + end):
                w = live[2 * cur + end][0][0]
                if w >> 1 == r:
                    circular = True
                    break
                cur, end = w >> 1, 1 - (w & 1)
            if circular:
                cur, end = r, 0
            term0 = 2 * cur + end
            members, out, total = [cur], 1 - end, length[cur]
            while joined(2 * cur + out):
                w, e = live[2 * cur + out][0]
                if w >> 1 == members[0]:
                    break
                cur, out = w >> 1, 1 - (w & 1)
                members.append(cur)
                total += length[cur] - es[e]
            term1 = 2 * cur + out
            rec = {"reads": len(members), "length": total, "first": min(members), "members": members, "circular": circular, "terms": (term0, term1)}
            dead = [deg(term0) == 0, deg(term1) == 0]
            rec["candidate"] = (not circular) and dead[0] != dead[1] and len(members) <= T
            rec["attached"] = (term1 if dead[0] else term0) if rec["candidate"] else -1
            rec["isolated_short"] = (not circular) and dead[0] and dead[1] and len(members) <= T
            for x in members:
                of[x] = rec
        return of

    def beats(d, c):
        return (not d["candidate"]) or (d["reads"], d["length"], -d["first"]) > (c["reads"], c["length"], -c["first"])

    rounds_run = converged = tips = tip_reads = tip_bases = tip_edges = candidates_kept = 0
    for k in range(1, R + 1):
        live = live_rows()
        of = chains(live)
        fallen, kept_now = [], 0
        for rec in {id(c): c for c in of.values()}.values():
            if not rec["candidate"]:
                continue
            b = rec["attached"]
            if all(any(x != b and beats(of[x >> 1], rec) for x, _ in live.get(w, ())) for w, _ in live[b]):
                fallen.append(rec)
            else:
                kept_now += 1
        for rec in fallen:
            for r in rec["members"]:
                read_state[r], read_round[r] = 1, k
            tips, tip_reads, tip_bases = tips + 1, tip_reads + rec["reads"], tip_bases + rec["length"]
        for e in range(ne):
            if edge_state[e] == 0 and (read_state[eu[e] >> 1] == 1 or read_state[ew[e] >> 1] == 1):
                edge_state[e], edge_round[e] = TIP, k
                tip_edges += 1
        rounds_run, candidates_kept = k, kept_now
        if not fallen:
            converged = 1
            break
    live = live_rows()
    of = chains(live)
    kept = [len(live.get(u, ())) for u in range(2 * n)]
    partner, span, flags = [-1] * (2 * n), [0] * (2 * n), [0] * n
    for r in range(n):
        flags[r] = SKIPPED if read_state[r] != 0 else 0
        for end in range(2):
            u = 2 * r + end
            if kept[u] == 1 and kept[live[u][0][0]] == 1:
                w, e = live[u][0]
                partner[u], span[u] = w >> 1, es[e]
                flags[r] |= ((REV5 if (w & 1) == end else 0) | MUTUAL5) << (2 * end)
    stays = [read_state[r] == 0 for r in range(n)]
    summary = {
        "reads": n, "reads_flagged": sum(flagged), "edges": ne, "weak_arcs": sum(bin(s & 3).count("1") for s in edge_state),
        "weak_edges": sum(1 for s in edge_state if s & 3), "rounds_run": rounds_run, "converged": converged, "tips": tips, "tip_reads": tip_reads,
        "tip_bases": tip_bases, "tip_edges": tip_edges, "candidates_kept": candidates_kept,
        "isolated_short": sum(1 for c in {id(c): c for c in of.values()}.values() if c["isolated_short"]),
        "kept_edges": sum(1 for s in edge_state if s == 0), "ends_kept_one": sum(1 for k in kept if k == 1), "ends_kept_more": sum(1 for k in kept if k >= 2),
        "ends_mutual": sum(1 for p in partner if p >= 0), "ends_dead": sum(1 for u in range(2 * n) if stays[u >> 1] and kept[u] == 0),
        "longest_row": max(arcs, default=0),
    }
    if n == 0:
        summary.update(rounds_run=1, converged=1)
    u8, i32 = lambda a: np.array(a, np.uint8).reshape(-1), lambda a: np.array(a, np.int32).reshape(n, 2)
    return {"edge_state": u8(edge_state), "edge_round": u8(edge_round), "read_state": u8(read_state), "read_round": u8(read_round),
            "arcs": i32(arcs), "weak": i32(weak), "kept": i32(kept), "partner": i32(partner), "span": i32(span), "flags": u8(flags),
            "summary": summary, "error_index": -1}


class Layout:
    """An edge list built by hand: reads of one length, chains joined 3' -> 5'."""

    def __init__(self, read_len=1000):
        self.len, self.u, self.w, self.span, self.default_len = [], [], [], [], read_len

    def read(self, length=None):
        self.len.append(self.default_len if length is None else length)
        return len(self.len) - 1

    def reads(self, count, length=None):
        return [self.read(length) for _ in range(count)]

    def edge(self, u, w, span=500):
        self.u.append(u); self.w.append(w); self.span.append(span)
        return len(self.u) - 1

    def join(self, a, b, span=500):
        """3' of read a to 5' of read b"""
        return self.edge(2 * a + 1, 2 * b, span)

    def chain(self, reads, span=500):
        for a, b in zip(reads, reads[1:]):
            self.join(a, b, span)
        return reads

    def arrays(self, order=None, flip=None):
        """read_len, edge_u, edge_w, edge_span as int32 arrays; ``order`` permutes the edges, ``flip`` (booleans) exchanges u and w"""
        u, w, s = (np.array(a, np.int32).reshape(-1) for a in (self.u, self.w, self.span))
        if flip is not None:
            f = np.asarray(flip, bool)
            u, w = np.where(f, w, u).astype(np.int32), np.where(f, u, w).astype(np.int32)
        if order is not None:
            u, w, s = u[order], w[order], s[order]
        return np.array(self.len, np.int32).reshape(-1), np.ascontiguousarray(u), np.ascontiguousarray(w), np.ascontiguousarray(s)
