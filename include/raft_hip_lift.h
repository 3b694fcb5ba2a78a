/* raft_hip_lift.h -- the overlaps between the fragments: every record of a stream cut at the fragment bounds of both of its reads and
 * shifted into fragment coordinates, in libraft_hip_lift.so.
 *
 * The entry points of raft_hip.h are a closed set (ABI 11).  This call ships beside them, in a library of its own built from the
 * same tree, as raft_hip_frag.h and the eight others do: it takes the context raft_hip_create made.  Link -lraft_hip_lift -lraft_hip.
 * raft_hip_lift_abi() returns the RAFT_HIP_ABI_VERSION the library was built beside; a caller checks it against
 * raft_hip_abi_version() once. */
#ifndef RAFT_HIP_LIFT_H
#define RAFT_HIP_LIFT_H
#include "raft_hip_frag.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

int raft_hip_lift_abi(void);

/*  * The table is raft_hip_frag_table with the semantics of raft_hip_frag.h: the same check on the device (a violation is
 * RAFT_HIP_ERR_PARAM, and no record and no row is read then), explicit arrays in any state of the context, or all NULL with
 * n_frag == -1 for the context's own finished pass (otherwise RAFT_HIP_ERR_STATE; n_reads must be that pass's, otherwise
 * RAFT_HIP_ERR_PARAM).  F(r) are the rows of read r, row k the half-open interval [fb[k], fe[k]).
 *
 * The rule.  A record (qid, qs, qe, tid, ts, te, rev) -- rev = strand[i] != 0, the strand byte of raft_hip_end.h -- lifts to nothing
 * when qid == tid, qe <= qs or te <= ts.  All arithmetic is in 64-bit integers; with coordinates in [0, 2^31) the largest product
 * is (vb + 1) * LA, at most 2^62.
 *   Canonical side.  A is the side of the read with the smaller id, [as, ae) on read a; B is the other side, [bs, be) on read b;
 *     LA = ae - as, LB = be - bs.  (Interpolating from the canonical side makes a record and its mirror lift to mirror images.)
 *   Rows.  Row i of F(a) is touched when fe[i] > as && fb[i] < ae; row j of F(b) is touched when fe[j] > bs && fb[j] < be.
 *   Pairs.  Every pair (i, j) of touched rows, i ascending, then j ascending:
 *     1. ua = max(0, fb[i] - as), ub = min(LA, fe[i] - as)
 *     2. rev == 0: va = max(0, fb[j] - bs), vb = min(LB, fe[j] - bs)
 *     3. rev == 1: va = max(0, be - fe[j]), vb = min(LB, be - fb[j])
 *     4. u1 = max(ua, ceil(va * LA / LB))
 *     5. u2 = min(ub, ceil((vb + 1) * LA / LB) - 1)
 *     6. the pair is dropped when u2 - u1 < min_len
 *     7. v1 = floor(u1 * LB / LA), v2 = floor(u2 * LB / LA)
 *     8. the pair is dropped when v2 - v1 < min_len
 *     (va <= v1 <= v2 <= vb follows from 4, 5 and 7.)
 *   Emitted record, in coordinates relative to the rows:
 *     A side: row i, [as + u1 - fb[i], as + u2 - fb[i])
 *     B side: row j, rev == 0: [bs + v1 - fb[j], bs + v2 - fb[j]);  rev == 1: [be - v2 - fb[j], be - v1 - fb[j])
 *     The sides go back into query and target order; rev is kept (as 0 or 1); src is the record's index.
 *   Rows are global row indices (read_num - 1 of PREFIX.reads.fasta).  Outputs are ordered by record, then in the order above.
 *   min_len >= 1.  Nothing is an error in a coordinate: sides are clipped by the rows.
 *
 * Outputs.  Eight columns of n_out elements: qfrag, qs, qe, tfrag, ts, te (int32), rev (uint8), src (int32) -- the caller's DEVICE
 * arrays in the _device form, host arrays in the _host form, of out_cap elements each.  Any may be NULL.  They are written only when
 * summary->n_out <= out_cap; otherwise the code is RAFT_HIP_ERR_TOO_LARGE, nothing is written and n_out says what is needed.  The
 * size query, all eight NULL, always succeeds (the conventions of raft_hip_low.h).  The summary is host memory in both forms.
 *
 * Errors.  An id outside [0, n_reads) -> RAFT_HIP_ERR_READ_ID with *error_index the first such record; otherwise *error_index = -1.
 * n_rec >= 2^30, n_frag >= 2^31 - 1 or n_out >= 2^31 - 1 -> RAFT_HIP_ERR_TOO_LARGE.  A missing column (the six and strand, whenever
 * n_rec > 0), min_len < 1, a negative count (other than the -1 above), out_cap < 0 -> RAFT_HIP_ERR_PARAM.  No output is written on
 * any error.
 *
 * The _host form stages its arguments through buffers of the context that no pass uses.  One wait inside the call: the host reads
 * n_out before the outputs are written.  kernel_seconds (may be NULL): device time of the launches, from events on the stream. */
typedef struct raft_hip_lift_summary {
    int64_t n_records;
    int64_t n_out;                                     /* outputs of the whole stream */
    int64_t records_none;                              /* records without an output */
    int64_t records_cut;                               /* records with more than one */
    int64_t pairs_dropped;                             /* pairs of touched rows dropped under min_len */
    int64_t most_per_record;                           /* the most outputs of one record */
} raft_hip_lift_summary;

/* `records` is raft_hip_records of raft_hip.h: n_rec and the six columns. */
int raft_hip_lift_overlaps_device(raft_hip_ctx *ctx, int32_t n_reads, const raft_hip_records *records, const uint8_t *d_strand,
                                  const raft_hip_frag_table *table, int32_t min_len, int64_t out_cap, int32_t *d_qfrag, int32_t *d_qs,
                                  int32_t *d_qe, int32_t *d_tfrag, int32_t *d_ts, int32_t *d_te, uint8_t *d_rev, int32_t *d_src,
                                  raft_hip_lift_summary *summary, int64_t *error_index, double *kernel_seconds);
int raft_hip_lift_overlaps_host(raft_hip_ctx *ctx, int32_t n_reads, const raft_hip_records *records, const uint8_t *strand,
                                const raft_hip_frag_table *table, int32_t min_len, int64_t out_cap, int32_t *qfrag, int32_t *qs,
                                int32_t *qe, int32_t *tfrag, int32_t *ts, int32_t *te, uint8_t *rev, int32_t *src,
                                raft_hip_lift_summary *summary, int64_t *error_index, double *kernel_seconds);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
