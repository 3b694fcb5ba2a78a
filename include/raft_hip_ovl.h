/* raft_hip_ovl.h -- which overlaps lie inside repeats: the record stream classified against the repeat annotation, in
 * libraft_hip_ovl.so.
 *
 * The entry points of raft_hip.h are a closed set (ABI 11).  This query ships beside them, in a library of its own built from the
 * same tree, as raft_hip_low.h does: it takes the context raft_hip_create made.  Link -lraft_hip_ovl -lraft_hip.
 * raft_hip_ovl_abi() returns the RAFT_HIP_ABI_VERSION the library was built beside; a caller checks it against
 * raft_hip_abi_version() once. */
#ifndef RAFT_HIP_OVL_H
#define RAFT_HIP_OVL_H
#include "raft_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

int raft_hip_ovl_abi(void);

/*  * Definitions.  For read r let runs(r) be the intervals [rep_s[k], rep_e[k]) for rep_offset[r] <= k < rep_offset[r + 1].  Within a
 * read rep_s is non-decreasing; rep_e need not be, flanks make neighbouring runs overlap, and runs clamped to start 0 tie on rep_s
 * in no particular order.  Everything below is therefore defined on the SET UNION U(r) of the runs, never on a per-run sum.
 * For one side [a, b) of a record on read r:
 *     span   = max(b - a, 0)
 *     rep    = |[a, b) intersected with U(r)|
 *     unique = span - rep                       (64-bit: span can be 2^31 - 1 and more)
 * Coordinates are taken as they are: nothing is clipped to the read's length and no coordinate is an error.
 *
 * Class byte of record i (both sides are classified always, whatever `symmetric` says):
 *     RAFT_HIP_OVL_Q_REPEAT     query side:  rep > 0 and unique < min_anchor
 *     RAFT_HIP_OVL_T_REPEAT     target side: the same
 *     RAFT_HIP_OVL_Q_TOUCH      query side:  rep > 0
 *     RAFT_HIP_OVL_T_TOUCH      target side: rep > 0
 *     RAFT_HIP_OVL_Q_CONTAINED  qs == 0 && qe == len[qid] && len[tid] > len[qid]      (the census's rule)
 *     RAFT_HIP_OVL_T_CONTAINED  ts == 0 && te == len[tid] && len[qid] > len[tid]
 * The target columns ts / te may be NULL only when symmetric != 0; the three target bits are then 0.
 *
 * Per read, sides counted exactly as intervals[] of raft_hip_census_* counts them: every query side of a record with qid == r and,
 * when symmetric == 0, every target side of a record with tid == r && tid != qid.
 *     read_touch[r], read_repeat[r]  (int32) the sides of r that have TOUCH / REPEAT
 *     read_flags[r]  (uint8)  RAFT_HIP_OVL_READ_CONTAINED  a counted side of r has CONTAINED (the census's flags != 0)
 *                             RAFT_HIP_OVL_READ_ANCHORED   some such record's CONTAINER side (the other side) is not REPEAT
 * A read with read_flags == RAFT_HIP_OVL_READ_CONTAINED is repeat-contained: every overlap that contains it places it inside a
 * repeat of the container.
 *
 * The repeat annotation is an argument.  All three arrays NULL with n_rep == -1: the context's own finished pass -- valid exactly
 * where raft_hip_read_stats is (otherwise RAFT_HIP_ERR_STATE), n_reads must be that pass's (otherwise RAFT_HIP_ERR_PARAM); nothing
 * of the pass is written and no geometry is handed out.  With explicit arrays (device arrays in the _device form, host arrays in
 * the _host form; rep_offset int64 [n_reads + 1], rep_s / rep_e int32 [n_rep]) the call is valid in any state of the context; a
 * pass in flight on the stream is waited for.  Some but not all of the three NULL -> RAFT_HIP_ERR_PARAM.  The kernel that walks the
 * reads checks rep_offset[0] == 0, rep_offset[r] <= rep_offset[r + 1] and rep_offset[n_reads] == n_rep: a violation is
 * RAFT_HIP_ERR_PARAM, and the record kernel reads no record and no run (every workgroup leaves at its first instruction).
 *
 * min_anchor < 1, a negative count or a missing column -> RAFT_HIP_ERR_PARAM.  An id outside [0, n_reads) ->
 * RAFT_HIP_ERR_READ_ID with *error_index the first such record (either column); no output is written.  Otherwise *error_index = -1.
 *
 * Outputs: cls is n_rec bytes -- the caller's DEVICE array in the _device form, a host array in the _host form; read_touch,
 * read_repeat, read_flags [n_reads] and sum are host memory in both forms.  Any output may be NULL.  The _host form stages its
 * arguments through buffers of the context that no pass uses, as raft_hip_census_host does.  kernel_seconds (may be NULL): device
 * time of the launches. */
#define RAFT_HIP_OVL_Q_REPEAT     1
#define RAFT_HIP_OVL_T_REPEAT     2
#define RAFT_HIP_OVL_Q_TOUCH      4
#define RAFT_HIP_OVL_T_TOUCH      8
#define RAFT_HIP_OVL_Q_CONTAINED 16
#define RAFT_HIP_OVL_T_CONTAINED 32
#define RAFT_HIP_OVL_READ_CONTAINED 1
#define RAFT_HIP_OVL_READ_ANCHORED  2
typedef struct raft_hip_ovl_summary {
    int64_t n_records;                                 /* over the records: all of them, and those with the bit */
    int64_t q_touch, t_touch, q_repeat, t_repeat;
    int64_t both_repeat;                               /* Q_REPEAT and T_REPEAT */
    int64_t q_contained, t_contained;
    int64_t reads_contained;                           /* over the reads: read_flags & RAFT_HIP_OVL_READ_CONTAINED */
    int64_t reads_repeat_contained;                    /* read_flags == RAFT_HIP_OVL_READ_CONTAINED */
} raft_hip_ovl_summary;

int raft_hip_repeat_overlaps_device(raft_hip_ctx *ctx, int32_t n_reads, const int32_t *d_read_len, int64_t n_rec,
                                    const int32_t *d_qid, const int32_t *d_qs, const int32_t *d_qe,
                                    const int32_t *d_tid, const int32_t *d_ts, const int32_t *d_te,
                                    int32_t symmetric, int32_t min_anchor,
                                    int64_t n_rep, const int64_t *d_rep_offset, const int32_t *d_rep_s, const int32_t *d_rep_e,
                                    uint8_t *d_cls, int32_t *read_touch, int32_t *read_repeat, uint8_t *read_flags,
                                    raft_hip_ovl_summary *sum, int64_t *error_index, double *kernel_seconds);
int raft_hip_repeat_overlaps_host(raft_hip_ctx *ctx, int32_t n_reads, const int32_t *read_len, int64_t n_rec,
                                  const int32_t *qid, const int32_t *qs, const int32_t *qe,
                                  const int32_t *tid, const int32_t *ts, const int32_t *te,
                                  int32_t symmetric, int32_t min_anchor,
                                  int64_t n_rep, const int64_t *rep_offset, const int32_t *rep_s, const int32_t *rep_e,
                                  uint8_t *cls, int32_t *read_touch, int32_t *read_repeat, uint8_t *read_flags,
                                  raft_hip_ovl_summary *sum, int64_t *error_index, double *kernel_seconds);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
