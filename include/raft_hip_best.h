/* raft_hip_best.h -- the best overlap of every read end: per read and end the longest dovetail to a read that is not left out,
 * whether that choice is mutual, and the reads whose two ends are both mutual (the best overlap graph of Canu's bogart and of
 * miniasm's arc selection), in libraft_hip_best.so.
 *
 * The entry points of raft_hip.h are a closed set (ABI 11).  This call ships beside them, in a library of its own built from the
 * same tree, as raft_hip_low.h, raft_hip_ovl.h, raft_hip_frag.h, raft_hip_rst.h, raft_hip_flt.h and raft_hip_end.h do: it takes the
 * context raft_hip_create made.  Link -lraft_hip_best -lraft_hip.  raft_hip_best_abi() returns the RAFT_HIP_ABI_VERSION the library
 * was built beside; a caller checks it against raft_hip_abi_version() once.  Like overlap_ends it looks at no finished pass and is
 * valid in any state of the context, which it leaves as it is (a pass in flight on the stream is waited for). */
#ifndef RAFT_HIP_BEST_H
#define RAFT_HIP_BEST_H
#include "raft_hip_end.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

int raft_hip_best_abi(void);

/*  * The rule (integers only).  Records, read lengths, strand, H = max_overhang and F = min_ratio_permille are those of
 * raft_hip_end.h, and so is the kind of a record.  For read r and end E (0 = 5', 1 = 3') a view is a record seen from its query or,
 * unless symmetric != 0, the same record seen from its target (kinds 4 and 5 swap on '+' and stay on '-').  A view (me, other, kind,
 * rev) is a candidate for slot (me, E) if
 *
 *     kind is RAFT_HIP_END_QUERY_5 (E = 0) or RAFT_HIP_END_QUERY_3 (E = 1), and
 *     neither me nor other is flagged in skip (uint8 per read, any non-zero byte is a flag; skip == NULL: no read is flagged).
 *
 * A dovetail view with a flagged side is left out; every other kind adds nothing.  A candidate has the key
 *
 *     span = min(qe - qs, te - ts)                      (the same in both views)
 *     key  = (uint64)span << 33 | (uint64)(0x7FFFFFFF - other) << 2 | (uint64)rev << 1
 *
 * and the best overlap of a slot is the candidate with the greatest key: the longest span, then the smaller partner id, then '-'
 * before '+'.  Candidates with equal keys are indistinguishable in the output, so the table is a function of the multiset of records
 * and not of their order.  Key 0 is "no best overlap" (a valid record has span >= 1).  The partner's end is E' = rev ? E : 1 - E.
 * Slot (r, E) with best (p, rev) is mutual iff slot (p, E') has a best overlap whose partner is r and whose own partner end is E;
 * mutual ends come in pairs.  A record and its mirror (tid ts te qid qs qe rev) give the same views, so a symmetric stream counted
 * on its query sides alone gives the table of its half counted on both. */
#define RAFT_HIP_BEST_REV5 1      /* flags: the 5' end's best overlap is on '-' */
#define RAFT_HIP_BEST_MUTUAL5 2   /*        the 5' end's best overlap is mutual */
#define RAFT_HIP_BEST_REV3 4      /*        the same for the 3' end */
#define RAFT_HIP_BEST_MUTUAL3 8
#define RAFT_HIP_BEST_SKIPPED 16  /*        the read is flagged in skip */

/*  * raft_hip_best_summary: n_records = n_rec; candidates and left_out count views; ends_best the slots with a best overlap,
 * ends_mutual those of them that are mutual (an even number); reads_both_best and reads_both_mutual the reads with a best (a
 * mutual) overlap at both ends; reads_no_best the reads that are not flagged and have no best overlap at either end; reads_skipped
 * the flagged reads.
 *
 * _device: read_len, the six columns, strand (uint8 [n_rec]) and skip (uint8 [n_reads], may be NULL) are DEVICE arrays.  _host:
 * they are host arrays, staged by the library.  partner (int32 [2 * n_reads], index 2 * r + E, -1: none), span (int32
 * [2 * n_reads], 0: none), flags (uint8 [n_reads]), the summary, error_index and kernel_seconds are host memory in both forms and
 * may each be NULL; kernel_seconds is the device time of the launches, from events on the context's stream.  A read length below 0
 * counts as 0 (no record on such a read is valid).
 *
 * A record whose qid or tid lies outside [0, n_reads) is RAFT_HIP_ERR_READ_ID, with the smallest index of such a record in
 * *error_index (the query column is looked at first: one index, whichever of a record's two ids is out of range).  No output is
 * then written.  Without such a record *error_index is -1.
 *
 * Refused with RAFT_HIP_ERR_PARAM before any launch, with a message (raft_hip_last_error) that starts "best_overlaps:":
 * max_overhang < 0, min_ratio_permille outside [0, 1000], n_reads < 0, n_rec < 0, read_len missing while n_reads > 0, and with
 * n_rec > 0 a missing column (the six and strand).  n_rec == 0: every slot is empty. */
typedef struct raft_hip_best_summary {
    int64_t n_records;
    int64_t candidates;
    int64_t left_out;
    int64_t ends_best;
    int64_t ends_mutual;
    int64_t reads_both_best;
    int64_t reads_both_mutual;
    int64_t reads_no_best;
    int64_t reads_skipped;
} raft_hip_best_summary;

int raft_hip_best_overlaps_device(raft_hip_ctx *ctx, int32_t n_reads, const int32_t *d_read_len, int64_t n_rec, const int32_t *d_qid,
                                  const int32_t *d_qs, const int32_t *d_qe, const int32_t *d_tid, const int32_t *d_ts, const int32_t *d_te,
                                  const uint8_t *d_strand, const uint8_t *d_skip, int32_t max_overhang, int32_t min_ratio_permille,
                                  int32_t symmetric, int32_t *partner, int32_t *span, uint8_t *flags, raft_hip_best_summary *sum,
                                  int64_t *error_index, double *kernel_seconds);
int raft_hip_best_overlaps_host(raft_hip_ctx *ctx, int32_t n_reads, const int32_t *read_len, int64_t n_rec, const int32_t *qid,
                                const int32_t *qs, const int32_t *qe, const int32_t *tid, const int32_t *ts, const int32_t *te,
                                const uint8_t *strand, const uint8_t *skip, int32_t max_overhang, int32_t min_ratio_permille,
                                int32_t symmetric, int32_t *partner, int32_t *span, uint8_t *flags, raft_hip_best_summary *sum,
                                int64_t *error_index, double *kernel_seconds);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
