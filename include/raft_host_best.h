/* raft_host_best.h -- the host text layer's part of `raft --best-overlaps`: the writer of PREFIX.best_overlaps.tsv (libraft_host.so,
 * beside the functions of raft_host.h). */
#ifndef RAFT_HOST_BEST_H
#define RAFT_HOST_BEST_H
#include "raft_host.h"

#ifdef __cplusplus
extern "C" {
#endif

/* PREFIX.best_overlaps.tsv: one line per read in read order, no header, tab-separated:
 *     name  length  partner5  strand5  span5  mutual5  partner3  strand3  span3  mutual3  skipped
 * partner, span and flags are raft_hip_best_overlaps_*'s outputs (int32 [2 * n_reads] each, index 2 * r + E; uint8 [n_reads], the
 * bits RAFT_HIP_BEST_* of raft_hip_best.h).  A partner is written by its name, the strand as '+' or '-', mutual and skipped as 0 or
 * 1; an end without a best overlap (partner -1) is "*  *  0  0". */
int raft_host_write_best_overlaps(const char *path, const raft_host_reads *reads, const int32_t *partner, const int32_t *span, const uint8_t *flags);

#ifdef __cplusplus
}
#endif
#endif
