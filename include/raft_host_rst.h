/* raft_host_rst.h -- the host text layer's writer for `raft --repeat-stats` (libraft_host.so, beside the functions of raft_host.h). */
#ifndef RAFT_HOST_RST_H
#define RAFT_HOST_RST_H
#include "raft_host.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The table of `raft --repeat-stats` (PREFIX.long_repeats.stats.tsv), from the repeat runs and what raft_hip_repeat_stats_* gives
 * (include/raft_hip_rst.h).  Tab-separated, no header line, names as they are; one line per run in the order of long_repeats.txt
 * (read by read, a read's runs in the order of the arrays),
 *       name  start  end  where  windows  cov_sum  cov_min  cov_max  high_windows  touching  spanning  inside
 *   name = the name of the read the run belongs to; start / end = rep_s / rep_e; where = `empty` (RAFT_HIP_RST_EMPTY), else `whole`
 *   (AT_START and AT_END), `head` (AT_START), `tail` (AT_END) or `interior` (no flag); the other columns are run_windows,
 *   run_cov_sum, run_cov_min, run_cov_max, run_high, run_touch, run_span, run_inside.
 * rep_offset [n_reads + 1] must begin at 0 and not descend (otherwise RAFT_HOST_ERR_ARG, nothing written).  The lines are formatted
 * by the layer's worker threads in blocks of reads and written in order: the bytes do not depend on the number of threads. */
int raft_host_write_repeat_stats(const char *path, int32_t n_reads, const char *const *names, const int64_t *rep_offset,
                                 const int32_t *rep_s, const int32_t *rep_e, const uint8_t *run_flags, const int32_t *run_windows,
                                 const int64_t *run_cov_sum, const int32_t *run_cov_min, const int32_t *run_cov_max,
                                 const int32_t *run_high, const int32_t *run_touch, const int32_t *run_span, const int32_t *run_inside);

#ifdef __cplusplus
}
#endif
#endif
