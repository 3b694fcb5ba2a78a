/* raft_host_ovl.h -- the host text layer's writer for `raft --repeat-overlaps` (libraft_host.so, beside the functions of raft_host.h). */
#ifndef RAFT_HOST_OVL_H
#define RAFT_HOST_OVL_H
#include "raft_host.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The two tables of `raft --repeat-overlaps A`, from what raft_hip_repeat_overlaps_* gives (include/raft_hip_ovl.h).  Tab-separated, no
 * header line, names as they are.
 *   reads_path (PREFIX.repeat_overlaps.tsv): one line per read in read order,
 *       name  length  touching  in_repeat  contained
 *     touching = read_touch[r], in_repeat = read_repeat[r]; contained is "no" (read_flags without RAFT_HIP_OVL_READ_CONTAINED),
 *     "anchored" (with RAFT_HIP_OVL_READ_ANCHORED) or "repeat" (contained, and only inside repeats of its containers).
 *   records_path (PREFIX.repeat_overlaps.records.tsv): one line per record with cls & 3 != 0, in record order,
 *       qname  qs  qe  tname  ts  te  side  contained
 *     side is "query" (RAFT_HIP_OVL_Q_REPEAT alone), "target" (RAFT_HIP_OVL_T_REPEAT alone) or "both"; contained is "query"
 *     (RAFT_HIP_OVL_Q_CONTAINED), "target" (RAFT_HIP_OVL_T_CONTAINED) or "-".  ts / te may be NULL: "-" is written for both.
 * Either path may be NULL (that table is not written).  The lines are formatted by the layer's worker threads in blocks and written
 * in order: the bytes do not depend on the number of threads. */
int raft_host_write_repeat_overlaps(const char *reads_path, const char *records_path, int32_t n_reads, const char *const *names,
                                    const int32_t *read_len, const int32_t *read_touch, const int32_t *read_repeat,
                                    const uint8_t *read_flags, int64_t n_rec, const int32_t *qid, const int32_t *qs, const int32_t *qe,
                                    const int32_t *tid, const int32_t *ts, const int32_t *te, const uint8_t *cls);

#ifdef __cplusplus
}
#endif
#endif
