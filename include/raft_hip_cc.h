/* raft_hip_cc.h -- the connected components of the overlap graph: which reads a record stream ties together at all, under the rule
 * of raft_hip_end.h and a mask of its kinds; per read the component and the degree, per component its size, in libraft_hip_cc.so.
 *
 * The entry points of raft_hip.h are a closed set (ABI 11).  This call ships beside them, in a library of its own built from the
 * same tree, as raft_hip_lift.h and the eight before it do: it takes the context raft_hip_create made.  Link -lraft_hip_cc
 * -lraft_hip.  raft_hip_cc_abi() returns the RAFT_HIP_ABI_VERSION the library was built beside; a caller checks it against
 * raft_hip_abi_version() once.  It looks at no finished pass and is valid in any state of the context, which it leaves as it is (a
 * pass in flight on the stream is waited for). */
#ifndef RAFT_HIP_CC_H
#define RAFT_HIP_CC_H
#include "raft_hip_end.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

int raft_hip_cc_abi(void);

/*  * The rule.  The input is that of raft_hip_overlap_ends_*: n_reads, read_len, the six columns, strand, H = max_overhang,
 * F = min_ratio_permille, symmetric -- and kind_mask, an int32 with bit k set for every kind k (RAFT_HIP_END_*) that counts as an edge.
 * Only the bits 1 .. 5 may be set and one of them must be. */
#define RAFT_HIP_CC_KINDS_PROPER 60     /* kinds 2, 3, 4, 5: the containments and the dovetails */
#define RAFT_HIP_CC_KINDS_ALL 62        /* kinds 1 .. 5: every overlap between two different reads, the internal matches included */

/*  * Edge.  A record is an edge when both of its ids lie in [0, n_reads) and its kind under the rule of raft_hip_end.h (as its query
 * sees it) is in the mask.  Invalid (0) and self (6) records are never edges.  PROPER and ALL hold a kind together with the kind its
 * mirror has, so under them a record is an edge exactly when its mirror is; a mask that holds 2 without 3, or 4 without 5, looks at
 * the record as written.
 *
 * Components.  The connected components of the undirected graph over ALL reads 0 .. n_reads - 1 with those edges; a read without an
 * edge is a component of one.  Component ids are dense, 0 .. C - 1, in the order of each component's smallest read id.  They do not
 * depend on the order of the records, on duplicates, or on whether a record's mirror is present.
 *
 * Per read: component (int32) and degree (int32).  Every edge record adds 1 to its query's degree and, unless symmetric != 0, 1 to
 * its target's -- the convention of raft_hip_end.h's counts: a mirrored stream counted on its query sides gives the table of its half
 * counted on both.
 *
 * Per component, C entries: comp_first (int32, the smallest read id), comp_reads (int32), comp_bases (int64, the sum of the lengths;
 * a length below 0 counts as 0) and comp_sides (int64, the sum of the degrees: twice the number of overlaps, under what symmetric
 * promises).
 *
 * raft_hip_cc_summary: n_reads; n_records = n_rec; edge_records the records that are edges; components = C; singletons the
 * components of one read; largest_reads and largest_bases the greatest comp_reads and the greatest comp_bases (not necessarily of
 * the same component); total_bases the sum of all lengths; reads_in_largest_permille = floor(1000 * largest_reads / n_reads), 0 when
 * n_reads == 0.
 *
 * _device: read_len, the six columns and strand (uint8 [n_rec]) are DEVICE arrays.  _host: they are host arrays, staged by the
 * library.  Every output is host memory in both forms and may be NULL: component and degree [n_reads]; comp_first, comp_reads,
 * comp_bases, comp_sides [n_reads] each, of which the call writes C entries (there are at most n_reads components, so a caller that
 * sizes them by n_reads never has to ask twice; what lies behind is left as it was); the summary, error_index, kernel_seconds (the
 * device time of the launches, from events on the context's stream) and launches (the number of kernels the call launched).
 *
 * A record whose qid or tid lies outside [0, n_reads) is RAFT_HIP_ERR_READ_ID, with the smallest index of such a record in
 * *error_index (the query column is looked at first: one index, whichever of a record's two ids is out of range).  No output but
 * error_index, kernel_seconds and launches is then written.  Without such a record *error_index is -1.
 *
 * Refused with RAFT_HIP_ERR_PARAM before any launch, with a message (raft_hip_last_error) that starts "components:": max_overhang < 0,
 * min_ratio_permille outside [0, 1000], n_reads < 0, n_rec < 0, read_len missing while n_reads > 0, with n_rec > 0 a missing
 * column (the six and strand), and a kind_mask that is 0 or has a bit other than 1 .. 5.  n_rec == 0: C = n_reads, every read alone. */
typedef struct raft_hip_cc_summary {
    int64_t n_reads;
    int64_t n_records;
    int64_t edge_records;
    int64_t components;
    int64_t singletons;
    int64_t largest_reads;
    int64_t largest_bases;
    int64_t total_bases;
    int64_t reads_in_largest_permille;
} raft_hip_cc_summary;

int raft_hip_components_device(raft_hip_ctx *ctx, int32_t n_reads, const int32_t *d_read_len, int64_t n_rec, const int32_t *d_qid,
                               const int32_t *d_qs, const int32_t *d_qe, const int32_t *d_tid, const int32_t *d_ts, const int32_t *d_te,
                               const uint8_t *d_strand, int32_t max_overhang, int32_t min_ratio_permille, int32_t kind_mask, int32_t symmetric,
                               int32_t *component, int32_t *degree, int32_t *comp_first, int32_t *comp_reads, int64_t *comp_bases,
                               int64_t *comp_sides, raft_hip_cc_summary *sum, int64_t *error_index, double *kernel_seconds,
                               int64_t *launches);
int raft_hip_components_host(raft_hip_ctx *ctx, int32_t n_reads, const int32_t *read_len, int64_t n_rec, const int32_t *qid,
                             const int32_t *qs, const int32_t *qe, const int32_t *tid, const int32_t *ts, const int32_t *te,
                             const uint8_t *strand, int32_t max_overhang, int32_t min_ratio_permille, int32_t kind_mask, int32_t symmetric,
                             int32_t *component, int32_t *degree, int32_t *comp_first, int32_t *comp_reads, int64_t *comp_bases,
                             int64_t *comp_sides, raft_hip_cc_summary *sum, int64_t *error_index, double *kernel_seconds,
                             int64_t *launches);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
