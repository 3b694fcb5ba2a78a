/* raft_hip_sg.h -- the string graph of a record stream: the dovetails between the reads that are not left out, one arc per pair of
 * read ends, without the arcs that two shorter arcs already imply (Myers' transitive reduction); per read end the arcs and the arcs
 * that survive, a table raft_hip_unitigs_* takes, and the list of edges, in libraft_hip_sg.so.
 *
 * The entry points of raft_hip.h are a closed set (ABI 11).  This call ships beside them, in a library of its own built from the
 * same tree, as raft_hip_cc.h and the ten before it do: it takes the context raft_hip_create made.  Link -lraft_hip_sg -lraft_hip.
 * raft_hip_sg_abi() returns the RAFT_HIP_ABI_VERSION the library was built beside; a caller checks it against
 * raft_hip_abi_version() once.  It looks at no finished pass and is valid in any state of the context, which it leaves as it is (a
 * pass in flight on the stream is waited for). */
#ifndef RAFT_HIP_SG_H
#define RAFT_HIP_SG_H
#include "raft_hip_best.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

int raft_hip_sg_abi(void);

/*  * The rule (integers only).  The input is that of raft_hip_best_overlaps_*: n_reads, read_len, the six columns, strand, skip (uint8
 * per read, any non-zero byte is a flag, NULL: no read is flagged), H = max_overhang, F = min_ratio_permille and symmetric -- and
 * fuzz (Z >= 0), emit_removed and out_cap.
 *
 * Nodes.  Node u = 2 * r + E is end E of read r (0 = 5', 1 = 3'); u ^ 1 is the read's other end.
 *
 * Views and arcs.  A view is a record as its query sees it and, unless symmetric != 0, its mirror (tid ts te qid qs qe rev) as its
 * own query sees it.  With q5 = qs, q3 = lq - qe, t5 = rev ? lt - te : ts, t3 = rev ? ts : lt - te of the view (raft_hip_end.h):
 *
 *     kind RAFT_HIP_END_QUERY_3:  u = 2 * me + 1,  ext = t3 - q3,  back = q5 - t5
 *     kind RAFT_HIP_END_QUERY_5:  u = 2 * me + 0,  ext = t5 - q5,  back = q3 - t3
 *     w = 2 * other + E',  E' = rev ? E : 1 - E,   span = min(qe - qs, te - ts)
 *
 * if neither read is flagged in skip.  ext is what the other read adds beyond the end, back what this read keeps beyond the other
 * read's far end; both are at least 1 for a dovetail kind.  A record's two views give twin arcs (u, w, ext, back, span) and
 * (w, u, back, ext, span).  A dovetail view with a flagged side is counted as left out; every other kind gives nothing.
 *
 * One arc per (u, w).  Among the arcs with the same (u, w) the one with the greatest key (span, -ext_lo, -ext_hi) stands; ext_lo is
 * the ext of the direction that leaves the read with the smaller id, ext_hi the other direction's.  An arc and its twin have the
 * same key, so twins are chosen from the same records, and arcs with equal keys are identical: the chosen set is a function of the
 * multiset of records, not of their order.  The row of u is the chosen arcs that leave u.
 *
 * Reducible.  Arc u -> w is reducible when the row of u holds an arc u -> v with v != w, ext(u -> v) < ext(u -> w), the row of v ^ 1
 * holds an arc to w, and |ext(u -> v) + ext(v ^ 1 -> w) - ext(u -> w)| <= Z.  Every arc is judged against the chosen set as it
 * stands, none against what another judgement left: the flags do not depend on an order of marking.  This departs from miniasm's
 * asg_arc_del_trans, which accepts any w reached within ext(u -> longest) + Z over a path (one-sided) and marks in the order of its
 * walk: there an arc that a much shorter path merely shadows falls, and which of two nearly equal arcs falls depends on the order.
 * The strict "nearer" test means two arcs of one end never remove each other; the two-sided bound keeps the shadowed arc.
 *
 * Edges.  The arcs u -> w and w -> u are one edge {u, w}; it is removed when either arc is reducible.  An arc whose twin is not in
 * the chosen set is unpaired and stands or falls by its own flag; that happens only when symmetric promised a mirror the stream
 * does not hold.  kept[u] is the number of arcs of u's row whose edge survives.
 *
 * The unitig table: partner, span [2 * n_reads] and flags [n_reads] in the layout raft_hip_unitigs_* takes (RAFT_HIP_BEST_*).  End u
 * is MUTUAL exactly when kept[u] == 1, its surviving arc u -> w has kept[w] == 1, the surviving arc of w is w -> u, and both carry
 * the same span (twins always do).  REV is E' == E; SKIPPED is set for a flagged read; an end that is not mutual holds -1 / 0 and no
 * REV bit.  The table passes raft_hip_unitigs_*'s consistency check by construction: a flagged read has no arc, so neither a MUTUAL
 * end nor a mutual partner is SKIPPED; w comes from a record with two valid ids that is no self overlap, so the partner lies in
 * [0, n_reads) and is not r; MUTUAL at u is decided by a test that is symmetric in u and w, so the partner's end E' has MUTUAL, its
 * partner is r and, since E' == E holds for both or neither, the same REV bit; the spans are equal by that test, and a valid record
 * has 1 <= span <= both lengths.
 *
 * The edge list: edge_u, edge_w, edge_span, edge_ext, edge_back (int32) and edge_flags (uint8, RAFT_HIP_SG_EDGE_*).  An edge is listed
 * once, as the arc u -> w that leaves the read with the smaller id (ext and back are that arc's); an unpaired arc is listed as it
 * is, with UNPAIRED.  The list is in ascending (u, w).  emit_removed == 0 lists the surviving edges, anything else every edge.
 * The list is written only when n_out <= out_cap; otherwise the call returns RAFT_HIP_ERR_TOO_LARGE, writes no array at all -- only
 * *n_out, the summary, error_index, kernel_seconds and launches -- and *n_out says what is needed (the contract of raft_hip_lift.h).
 * A call with all six edge arrays NULL is the size query: out_cap is not looked at and everything else is written. */
#define RAFT_HIP_SG_EDGE_RED_U 1      /* edge_flags: the arc u -> w is reducible */
#define RAFT_HIP_SG_EDGE_RED_W 2      /*             the arc w -> u is reducible */
#define RAFT_HIP_SG_EDGE_UNPAIRED 4   /*             the arc w -> u is not in the chosen set */

/*  * raft_hip_sg_summary: records = n_rec; dovetail_views the views that give an arc, views_left_out the dovetail views with a flagged
 * side; arcs the chosen arcs, duplicate_arcs = dovetail_views - arcs, unpaired_arcs and reducible_arcs those of the chosen arcs;
 * edges the edges as listed with emit_removed, removed_edges and kept_edges the two parts of them; ends_with_arc the nodes with a
 * row, ends_kept_one and ends_kept_more the nodes with kept == 1 and kept >= 2, ends_mutual the MUTUAL ends; ends_dead the ends of
 * reads that are not flagged with kept == 0; reads_flagged; longest_row the greatest row length.
 *
 * _device: read_len, the six columns, strand (uint8 [n_rec]) and skip (uint8 [n_reads], may be NULL) are DEVICE arrays.  _host: they
 * are host arrays, staged by the library.  Every output is host memory in both forms and may be NULL: arcs and kept (int32
 * [2 * n_reads]); partner, span (int32 [2 * n_reads]), flags (uint8 [n_reads]); the six edge arrays [out_cap]; n_out; the summary;
 * error_index; kernel_seconds (the device time of the launches, from events on the context's stream: two spans, the call waits once
 * for the number of views, which sizes the sort) and launches (the number of kernels the call launched).  The reduction's work is
 * the sum over the rows of the row length squared: longest_row and launches explain a slow call.
 *
 * A record whose qid or tid lies outside [0, n_reads) is RAFT_HIP_ERR_READ_ID, with the smallest index of such a record in
 * *error_index; no output but error_index, kernel_seconds and launches is then written.  Without such a record *error_index is -1.
 *
 * Refused before any launch, with a message (raft_hip_last_error) that starts "string_graph:": RAFT_HIP_ERR_PARAM for max_overhang < 0,
 * min_ratio_permille outside [0, 1000], n_reads < 0, n_rec < 0, read_len missing while n_reads > 0, with n_rec > 0 a missing column
 * (the six and strand), fuzz < 0 and out_cap < 0; RAFT_HIP_ERR_TOO_LARGE for n_reads > 2^30 - 1 or n_rec >= 2^30 (nodes and views
 * are int32).  n_rec == 0: every row is empty and there is no edge. */
typedef struct raft_hip_sg_summary {
    int64_t records;
    int64_t dovetail_views;
    int64_t views_left_out;
    int64_t arcs;
    int64_t duplicate_arcs;
    int64_t unpaired_arcs;
    int64_t reducible_arcs;
    int64_t edges;
    int64_t removed_edges;
    int64_t kept_edges;
    int64_t ends_with_arc;
    int64_t ends_kept_one;
    int64_t ends_kept_more;
    int64_t ends_mutual;
    int64_t ends_dead;
    int64_t reads_flagged;
    int64_t longest_row;
} raft_hip_sg_summary;

int raft_hip_string_graph_device(raft_hip_ctx *ctx, int32_t n_reads, const int32_t *d_read_len, int64_t n_rec, const int32_t *d_qid,
                                 const int32_t *d_qs, const int32_t *d_qe, const int32_t *d_tid, const int32_t *d_ts, const int32_t *d_te,
                                 const uint8_t *d_strand, const uint8_t *d_skip, int32_t max_overhang, int32_t min_ratio_permille,
                                 int32_t symmetric, int32_t fuzz, int32_t emit_removed, int64_t out_cap, int32_t *arcs, int32_t *kept,
                                 int32_t *partner, int32_t *span, uint8_t *flags, int32_t *edge_u, int32_t *edge_w, int32_t *edge_span,
                                 int32_t *edge_ext, int32_t *edge_back, uint8_t *edge_flags, int64_t *n_out, raft_hip_sg_summary *sum,
                                 int64_t *error_index, double *kernel_seconds, int64_t *launches);
int raft_hip_string_graph_host(raft_hip_ctx *ctx, int32_t n_reads, const int32_t *read_len, int64_t n_rec, const int32_t *qid,
                               const int32_t *qs, const int32_t *qe, const int32_t *tid, const int32_t *ts, const int32_t *te,
                               const uint8_t *strand, const uint8_t *skip, int32_t max_overhang, int32_t min_ratio_permille,
                               int32_t symmetric, int32_t fuzz, int32_t emit_removed, int64_t out_cap, int32_t *arcs, int32_t *kept,
                               int32_t *partner, int32_t *span, uint8_t *flags, int32_t *edge_u, int32_t *edge_w, int32_t *edge_span,
                               int32_t *edge_ext, int32_t *edge_back, uint8_t *edge_flags, int64_t *n_out, raft_hip_sg_summary *sum,
                               int64_t *error_index, double *kernel_seconds, int64_t *launches);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
