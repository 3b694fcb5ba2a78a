/* raft_hip_cln.h -- a string graph cleaned on the device: the edges that are weak beside the best one at the same read end are cut,
 * then the short dead-end chains (tips) that hang beside something greater are removed over several rounds; per edge and per read
 * what fell and when, per read end the degrees, and a table raft_hip_unitigs_* takes, in libraft_hip_cln.so.
 *
 * The entry points of raft_hip.h are a closed set (ABI 11).  This call ships beside them, in a library of its own built from the
 * same tree, as raft_hip_sg.h and the twelve before it do: it takes the context raft_hip_create made.  Link -lraft_hip_cln -lraft_hip.
 * raft_hip_cln_abi() returns the RAFT_HIP_ABI_VERSION the library was built beside; a caller checks it against
 * raft_hip_abi_version() once.  It looks at no finished pass and is valid in any state of the context, which it leaves as it is (a
 * pass in flight on the stream is waited for). */
#ifndef RAFT_HIP_CLN_H
#define RAFT_HIP_CLN_H
#include "raft_hip_best.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

int raft_hip_cln_abi(void);

/*  * The rule (integers only).
 *
 * Input.  n_reads and read_len; skip (uint8 per read, any non-zero byte flags the read, NULL: no read is flagged); an edge list of
 * n_edges rows edge_u, edge_w, edge_span.  Nodes are those of raft_hip_sg.h: u = 2 * r + E is end E of read r (0 = 5', 1 = 3').  Each
 * row is one undirected edge and gives both arcs, u -> w and w -> u, with that span.  The list may be in any order and either
 * orientation; the surviving list of raft_hip_string_graph_* is a valid input, and an UNPAIRED row there counts as a full edge here.
 * Parameters: W = min_ratio_permille in [0, 1000], T = max_tip_reads >= 0, R = rounds in [1, 64].
 *
 * The list is not trusted.  An edge is bad when u or w lies outside [0, 2 * n_reads), when u >> 1 == w >> 1, when either read is
 * flagged, when the span is below 1 or greater than the shorter of the two lengths (a negative length counts as 0), or when its
 * unordered pair {u, w} also stands at a smaller index.  A bad edge makes the call return RAFT_HIP_ERR_READ_ID with the smallest
 * index of a bad edge in *error_index; no output other than error_index, kernel_seconds and launches is then written.  Without one
 * *error_index is -1.
 *
 * Weak cut.  It runs once, before the rounds, and is judged against the list as given.  m(u) is the greatest span of an arc that
 * leaves u.  Arc u -> w is weak when span * 1000 < W * m(u), the products taken in 64 bits.  An edge falls when either of its arcs
 * is weak.  W = 0 cuts nothing.  The flag of one arc is never an input to another's.
 *
 * Tip rounds.  Round k = 1 .. R looks at the live graph: the reads that are neither flagged nor removed and the edges that have not
 * fallen.  deg(u) is the number of live arcs leaving u.  End u is joined when deg(u) == 1 and its arc u -> w has deg(w) == 1 -- the
 * MUTUAL test of raft_hip_sg.h.  A chain is a maximal set of live reads connected through joined ends; a read with no joined end
 * is a chain of one.  A chain whose ends are all joined is circular; every other chain has two terminal ends.  Per chain C:
 * reads(C); length(C) by the layout rule of raft_hip_utg.h (every read adds its length less the span to the next); first(C), its
 * smallest read id.  C is a candidate when it is not circular, exactly one terminal end has deg == 0, and reads(C) <= T; the other
 * terminal end, b, is its attached end.  D beats candidate C when D is no candidate, or when both are candidates and
 * (reads, length, -first) of D is lexicographically greater: among candidates a strict total order, since first differs between
 * chains.  Candidate C falls when, for every live arc b -> w, node w has a live arc w -> x with x != b whose read's chain beats C.
 * Every read of a fallen chain is removed, with every live edge that touches it.  All chains are judged against the graph as the
 * round found it.  The rounds stop after R, or after a round in which nothing fell; that round is counted in rounds_run, and
 * converged is 1.  T = 0 makes no chain a candidate.
 *
 * The result depends on no order.  The weak flags are functions of the given set, a round is a function of the live set, and "beats"
 * is strict, so two candidates never remove each other.  The invariant: where a read stays and has a node w that lost an attached
 * chain in a round, w keeps at least one live arc after that round -- the greatest chain at w is either no candidate, and then it
 * stays, or it is beaten by nothing at w, and then it cannot fall.  A round therefore never turns a node with arcs into a dead end.
 *
 * Two departures from miniasm.  asg_cut_tip deletes as it walks, so at a fork of two spurs which one survives depends on the vertex
 * order; here the greater one stays.  asg_cut_tip also deletes short chains that are dead at both ends; here they stay, and the
 * summary counts them (isolated_short).  (The weak cut is asg_arc_del_short's test with its ratio as W per mille, judged per arc
 * against the given list rather than in the order of a walk.)
 *
 * Outputs.  edge_state (uint8 [n_edges], in the caller's order): RAFT_HIP_CLN_WEAK_U the arc u -> w is weak, RAFT_HIP_CLN_WEAK_W the
 * arc w -> u is, RAFT_HIP_CLN_TIP the edge touched a read that was removed; 0: the edge stays.  edge_round (uint8): 0 for an edge that
 * stays or was cut weak, else the round in which it fell.  read_state (uint8 [n_reads]): 0 stays, 1 tip, 2 flagged; read_round
 * (uint8): the round in which a tip was removed, else 0.  Per end, [2 * n_reads] int32 each: arcs, the degree in the given list;
 * weak, the arcs of the end whose edge the weak cut removed; kept, the live degree at the end of the call.
 *
 * The unitig table: partner, span [2 * n_reads] and flags [n_reads] in the layout raft_hip_unitigs_* takes (RAFT_HIP_BEST_*).  SKIPPED
 * is set for flagged reads and for removed reads.  End u is MUTUAL exactly where it is joined in the final graph; REV is E' == E; an
 * end that is not mutual holds -1 / 0 and no REV bit.  The table passes raft_hip_unitigs_*'s consistency check by construction: a
 * live edge touches no flagged read (such an edge is bad) and no removed read (its edges fell with it), so neither a MUTUAL end
 * nor its partner is SKIPPED; a good edge has both nodes in range and joins two different reads, so the partner lies in
 * [0, n_reads) and is not r; both arcs of an edge live and fall together, so "joined" is symmetric in u and w: the partner's end E'
 * has MUTUAL, its partner is r and, since E' == E holds for both or neither, the same REV bit; both arcs carry the edge's one span,
 * and a good edge has 1 <= span <= both lengths. */
#define RAFT_HIP_CLN_WEAK_U 1      /* edge_state: the arc u -> w is weak */
#define RAFT_HIP_CLN_WEAK_W 2      /*             the arc w -> u is weak */
#define RAFT_HIP_CLN_TIP 4         /*             a read of the edge was removed as part of a tip */
#define RAFT_HIP_CLN_READ_STAYS 0  /* read_state */
#define RAFT_HIP_CLN_READ_TIP 1
#define RAFT_HIP_CLN_READ_FLAGGED 2

/*  * raft_hip_cln_summary: reads = n_reads, reads_flagged; edges = n_edges; weak_arcs the arcs that are weak, weak_edges the edges with
 * one at least; rounds_run and converged; tips the chains that fell, tip_reads their reads, tip_bases the sum of their lengths,
 * tip_edges the edges that fell with them; candidates_kept the candidates of the last judged round that did not fall;
 * isolated_short the final chains with both terminal ends dead and reads <= T; kept_edges the edges that stay; ends_kept_one and
 * ends_kept_more the nodes with kept == 1 and kept >= 2, ends_mutual the MUTUAL ends, ends_dead the ends with kept == 0 of reads
 * that are neither flagged nor removed; longest_row the greatest degree in the given list.
 *
 * _device: read_len, skip (may be NULL) and the three edge columns are DEVICE arrays.  _host: they are host arrays, staged by the
 * library.  Every output is host memory in both forms and may be NULL.  kernel_seconds is the device time of the launches, from
 * events on the context's stream; the call waits once for the list's check, once per round for the number of chains that fell and
 * once at the end: R + 2 waits at most.  launches is the number of kernels the call launched.
 *
 * Refused before any launch, with a message (raft_hip_last_error) that starts "graph_clean:": RAFT_HIP_ERR_PARAM for
 * min_ratio_permille outside [0, 1000], max_tip_reads < 0, rounds outside [1, 64], n_reads < 0, n_edges < 0, read_len missing while
 * n_reads > 0 and an edge column missing while n_edges > 0; RAFT_HIP_ERR_TOO_LARGE for n_reads > 2^30 - 1 or n_edges >= 2^30 (nodes
 * and arcs are int32).  n_edges == 0 is valid: nothing falls and converged is 1 after one round. */
typedef struct raft_hip_cln_summary {
    int64_t reads;
    int64_t reads_flagged;
    int64_t edges;
    int64_t weak_arcs;
    int64_t weak_edges;
    int64_t rounds_run;
    int64_t converged;
    int64_t tips;
    int64_t tip_reads;
    int64_t tip_bases;
    int64_t tip_edges;
    int64_t candidates_kept;
    int64_t isolated_short;
    int64_t kept_edges;
    int64_t ends_kept_one;
    int64_t ends_kept_more;
    int64_t ends_mutual;
    int64_t ends_dead;
    int64_t longest_row;
} raft_hip_cln_summary;

int raft_hip_graph_clean_device(raft_hip_ctx *ctx, int32_t n_reads, const int32_t *d_read_len, const uint8_t *d_skip, int64_t n_edges,
                                const int32_t *d_edge_u, const int32_t *d_edge_w, const int32_t *d_edge_span, int32_t min_ratio_permille,
                                int32_t max_tip_reads, int32_t rounds, uint8_t *edge_state, uint8_t *edge_round, uint8_t *read_state,
                                uint8_t *read_round, int32_t *arcs, int32_t *weak, int32_t *kept, int32_t *partner, int32_t *span,
                                uint8_t *flags, raft_hip_cln_summary *sum, int64_t *error_index, double *kernel_seconds, int64_t *launches);
int raft_hip_graph_clean_host(raft_hip_ctx *ctx, int32_t n_reads, const int32_t *read_len, const uint8_t *skip, int64_t n_edges,
                              const int32_t *edge_u, const int32_t *edge_w, const int32_t *edge_span, int32_t min_ratio_permille,
                              int32_t max_tip_reads, int32_t rounds, uint8_t *edge_state, uint8_t *edge_round, uint8_t *read_state,
                              uint8_t *read_round, int32_t *arcs, int32_t *weak, int32_t *kept, int32_t *partner, int32_t *span,
                              uint8_t *flags, raft_hip_cln_summary *sum, int64_t *error_index, double *kernel_seconds, int64_t *launches);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
