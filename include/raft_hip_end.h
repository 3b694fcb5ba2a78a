/* raft_hip_end.h -- what kind of overlap every record of a stream is, and which end of each read the records support: an internal
 * match, a containment, a dovetail at the read's 5' or at its 3' end; per read five counts and a status, in libraft_hip_end.so.
 *
 * The entry points of raft_hip.h are a closed set (ABI 11).  This call ships beside them, in a library of its own built from the
 * same tree, as raft_hip_low.h, raft_hip_ovl.h, raft_hip_frag.h, raft_hip_rst.h and raft_hip_flt.h do: it takes the context
 * raft_hip_create made.  Link -lraft_hip_end -lraft_hip.  raft_hip_end_abi() returns the RAFT_HIP_ABI_VERSION the library was built
 * beside; a caller checks it against raft_hip_abi_version() once.  Like the census it looks at no finished pass and is valid in any
 * state of the context (a pass in flight on the stream is waited for). */
#ifndef RAFT_HIP_END_H
#define RAFT_HIP_END_H
#include "raft_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

int raft_hip_end_abi(void);

/*  * The rule (miniasm's ma_hit2arc classification, in integers).  A record is qid qs qe tid ts te rev: the six tokenised values and
 * the strand, rev = 1 iff PAF field 5 begins with '-' (raft_host_paf_parse_with of raft_host_end.h gives it as one byte per record;
 * any byte other than 0 counts as 1).  With len[] the read lengths, H = max_overhang >= 0 and F = min_ratio_permille in [0, 1000]:
 *
 *     lq = len[qid], lt = len[tid]
 *     invalid (0)  unless 0 <= qs < qe <= lq and 0 <= ts < te <= lt
 *     self    (6)  if qid == tid
 *     q5 = qs, q3 = lq - qe;   t5 = rev ? lt - te : ts;   t3 = rev ? ts : lt - te
 *     e5 = min(q5, t5), e3 = min(q3, t3), span = min(qe - qs, te - ts)
 *     internal (1) if e5 > H or e3 > H or (int64)span * 1000 < (int64)F * (span + e5 + e3)
 *     qin = q5 <= t5 and q3 <= t3;   tin = q5 >= t5 and q3 >= t3
 *     qin and tin: the shorter read is the contained one; equal lengths: the read with the larger id
 *     query contained (2) / target contained (3)
 *     otherwise a dovetail: q5 > t5 -> at the query's 3' end (4), else at its 5' end (5)
 *
 * Seen from the target 2 and 3 swap, 4 and 5 swap on '+' and stay on '-', and 0, 1 and 6 stay.  Two departures from miniasm, on
 * purpose: span is the shorter of the two sides, and the tie of two equal overhangs is broken by length and then by id.  With them
 * the kind of a record and the kind of its mirror (tid ts te qid qs qe rev) always agree under the target's view, so a symmetric
 * stream counted on its query sides alone gives the table of its half counted on both. */
#define RAFT_HIP_END_INVALID 0
#define RAFT_HIP_END_INTERNAL 1
#define RAFT_HIP_END_QUERY_CONTAINED 2
#define RAFT_HIP_END_TARGET_CONTAINED 3
#define RAFT_HIP_END_QUERY_3 4
#define RAFT_HIP_END_QUERY_5 5
#define RAFT_HIP_END_SELF 6

/*  * Per read r five int32 counts, counts[k * n_reads + r] with k = 0 internal, 1 contained_in, 2 contains, 3 end5, 4 end3: every
 * valid record that is not a self overlap adds 1 to one count of its query's row (kind 1 -> internal, 2 -> contained_in,
 * 3 -> contains, 5 -> end5, 4 -> end3) and, unless symmetric != 0, 1 to one count of its target's row under the target's view.
 * Per read one status byte: */
#define RAFT_HIP_END_READ_LINKED 0      /* none of the below: something extends either end */
#define RAFT_HIP_END_READ_CONTAINED 1   /* contained_in > 0 */
#define RAFT_HIP_END_READ_ISOLATED 2    /* else end5 == 0 and end3 == 0 */
#define RAFT_HIP_END_READ_DEAD5 3       /* else end5 == 0 */
#define RAFT_HIP_END_READ_DEAD3 4       /* else end3 == 0 */

/*  * raft_hip_end_summary: n_records = n_rec; the records by kind 0..6; the reads by status 0..4.
 *
 * _device: read_len, the six columns, strand (uint8 [n_rec]) and kinds (uint8 [n_rec]) are DEVICE arrays.  _host: they are host
 * arrays, staged by the library.  kinds may be NULL in both forms and is then not written.  counts (int32 [5 * n_reads]), status
 * (uint8 [n_reads]), the summary, error_index and kernel_seconds are host memory in both forms, as the census's outputs are, and
 * may each be NULL; kernel_seconds is the device time of the launches, from events on the context's stream.
 *
 * A record whose qid or tid lies outside [0, n_reads) is RAFT_HIP_ERR_READ_ID, with the smallest index of such a record in
 * *error_index (the query column is looked at first: one index, whichever of a record's two ids is out of range).  counts, status,
 * the summary and the host form's kinds are then not written; the device form's kinds array holds no result.  Without such a record
 * *error_index is -1.
 *
 * Refused with RAFT_HIP_ERR_PARAM before any launch, with a message (raft_hip_last_error) that names overlap_ends: max_overhang < 0,
 * min_ratio_permille outside [0, 1000], n_reads < 0, n_rec < 0, read_len missing while n_reads > 0, and with n_rec > 0 a missing
 * column (the six and strand).  n_rec == 0: every count is 0 and every read is isolated. */
typedef struct raft_hip_end_summary {
    int64_t n_records;
    int64_t kind_invalid;
    int64_t kind_internal;
    int64_t kind_query_contained;
    int64_t kind_target_contained;
    int64_t kind_end3;
    int64_t kind_end5;
    int64_t kind_self;
    int64_t reads_linked;
    int64_t reads_contained;
    int64_t reads_isolated;
    int64_t reads_dead5;
    int64_t reads_dead3;
} raft_hip_end_summary;

int raft_hip_overlap_ends_device(raft_hip_ctx *ctx, int32_t n_reads, const int32_t *d_read_len, int64_t n_rec, const int32_t *d_qid,
                                 const int32_t *d_qs, const int32_t *d_qe, const int32_t *d_tid, const int32_t *d_ts, const int32_t *d_te,
                                 const uint8_t *d_strand, int32_t max_overhang, int32_t min_ratio_permille, int32_t symmetric,
                                 int32_t *counts, uint8_t *status, uint8_t *d_kinds, raft_hip_end_summary *sum, int64_t *error_index,
                                 double *kernel_seconds);
int raft_hip_overlap_ends_host(raft_hip_ctx *ctx, int32_t n_reads, const int32_t *read_len, int64_t n_rec, const int32_t *qid,
                               const int32_t *qs, const int32_t *qe, const int32_t *tid, const int32_t *ts, const int32_t *te,
                               const uint8_t *strand, int32_t max_overhang, int32_t min_ratio_permille, int32_t symmetric,
                               int32_t *counts, uint8_t *status, uint8_t *kinds, raft_hip_end_summary *sum, int64_t *error_index,
                               double *kernel_seconds);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
