/* raft_hip_flt.h -- which records of a stream go into a job at all: a minimum identity and a minimum span, and the kept records as
 * six new columns in their order, in libraft_hip_flt.so.
 *
 * The entry points of raft_hip.h are a closed set (ABI 11).  This call ships beside them, in a library of its own built from the
 * same tree, as raft_hip_low.h, raft_hip_ovl.h, raft_hip_frag.h and raft_hip_rst.h do: it takes the context raft_hip_create made.
 * Link -lraft_hip_flt -lraft_hip.  raft_hip_flt_abi() returns the RAFT_HIP_ABI_VERSION the library was built beside; a caller checks
 * it against raft_hip_abi_version() once.  Unlike the queries of those headers it looks at no finished pass: it chooses what a pass,
 * the census and every query will see, and is valid in any state of the context (a pass in flight on the stream is waited for). */
#ifndef RAFT_HIP_FLT_H
#define RAFT_HIP_FLT_H
#include "raft_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

int raft_hip_flt_abi(void);

/*  * The rule.  A record is its six tokenised values qid, qs, qe, tid, ts, te and the two quality values matches and block: PAF
 * columns 10 and 11, residue matches and alignment block length, as int32 (raft_host_paf_parse_quality of raft_host_flt.h gives
 * them).  With P = min_identity_permille in [0, 1000] and L = min_span >= 0
 *
 *     identity_ok = P == 0 || (block > 0 && matches >= 0 && (int64)matches * 1000 >= (int64)P * block)
 *     span_ok     = L == 0 || ((int64)qe - qs >= L && (int64)te - ts >= L)
 *     keep        = identity_ok && span_ok
 *
 * This is the reference workflow's awk on columns 10 and 11 ($10 * 100.0 / $11 >= MINIDENTITY, with P = 10 * MINIDENTITY) in
 * integers, plus a span on both sides.  A ten-field PAF line is a record whose block is 0: it fails every P > 0.  Read ids are
 * copied, never used as indices, and no coordinate is an error here: range errors stay the business of the pass that gets the kept
 * stream.
 *
 * The kept records are written to the six output columns in their order: out_*[k] is the k-th kept record, k < summary.n_kept.
 * Every output column has room for n_rec values.  A job on the kept columns is the job on a file that holds exactly the kept lines.
 *
 * raft_hip_flt_summary:
 *     n_records       n_rec
 *     n_kept
 *     below_identity  records with identity_ok false
 *     below_span      records with span_ok false (a record may count in both)
 *     first_kept      index in the input of the first kept record, -1 when none is kept
 *     symmetric       what raft_host_paf_symmetric reports for the kept stream (chop.hpp:171-184): 1 iff some kept record other than
 *                     the first kept one has (qid, qs, qe, tid, ts, te) equal to the first kept record's (tid, ts, te, qid, qs, qe)
 *
 * _device: the eight input columns and the six output columns are DEVICE arrays; an output range [out, out + n_rec) that overlaps
 * an input column or another output is refused (RAFT_HIP_ERR_PARAM).  _host: all are host arrays; an output column may be the
 * input column itself (everything is staged before the first launch, and the copies back follow the wait), n_kept values each are
 * copied back.  The summary and kernel_seconds are host memory in both forms and may be NULL; kernel_seconds is the device time of
 * the launches, from events on the context's stream.
 *
 * Refused with RAFT_HIP_ERR_PARAM before any launch, with a message (raft_hip_last_error) that names filter_overlaps:
 * min_identity_permille outside [0, 1000], min_span < 0, n_rec < 0, and with n_rec > 0 a missing input or output column -- matches
 * and block may be NULL only when min_identity_permille == 0 (they are not read then).  n_rec == 0: nothing is launched. */
typedef struct raft_hip_flt_summary {
    int64_t n_records;
    int64_t n_kept;
    int64_t below_identity;
    int64_t below_span;
    int64_t first_kept;
    int64_t symmetric;
} raft_hip_flt_summary;

int raft_hip_filter_overlaps_device(raft_hip_ctx *ctx, int64_t n_rec, const int32_t *d_qid, const int32_t *d_qs, const int32_t *d_qe,
                                    const int32_t *d_tid, const int32_t *d_ts, const int32_t *d_te, const int32_t *d_matches,
                                    const int32_t *d_block, int32_t min_identity_permille, int32_t min_span,
                                    int32_t *d_out_qid, int32_t *d_out_qs, int32_t *d_out_qe, int32_t *d_out_tid, int32_t *d_out_ts,
                                    int32_t *d_out_te, raft_hip_flt_summary *sum, double *kernel_seconds);
int raft_hip_filter_overlaps_host(raft_hip_ctx *ctx, int64_t n_rec, const int32_t *qid, const int32_t *qs, const int32_t *qe,
                                  const int32_t *tid, const int32_t *ts, const int32_t *te, const int32_t *matches,
                                  const int32_t *block, int32_t min_identity_permille, int32_t min_span,
                                  int32_t *out_qid, int32_t *out_qs, int32_t *out_qe, int32_t *out_tid, int32_t *out_ts,
                                  int32_t *out_te, raft_hip_flt_summary *sum, double *kernel_seconds);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
