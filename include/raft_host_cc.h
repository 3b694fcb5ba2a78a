/* raft_host_cc.h -- the host text layer's part of `raft --components`: the writer of PREFIX.components.tsv and
 * PREFIX.components.summary.tsv (libraft_host.so, beside the functions of raft_host.h). */
#ifndef RAFT_HOST_CC_H
#define RAFT_HOST_CC_H
#include "raft_host.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Two files, no header line, tab-separated, from raft_hip_components_*'s outputs (include/raft_hip_cc.h) for the reads of `reads`:
 *     PREFIX.components.tsv          one line per read in read order:        name  length  component  degree
 *     PREFIX.components.summary.tsv  one line per component in id order:     component  reads  bases  sides  first_read
 * first_read is the name of the component's smallest read.  n_components is C; the per-read arrays are [n_reads], the per-component
 * arrays [C].  A table that names a component outside [0, C) or a first read outside the set is refused (RAFT_HOST_ERR_ARG) before
 * anything is written.  The bytes do not depend on the number of threads. */
int raft_host_write_components(const char *prefix, const raft_host_reads *reads, int64_t n_components, const int32_t *component,
                               const int32_t *degree, const int32_t *comp_first, const int32_t *comp_reads, const int64_t *comp_bases,
                               const int64_t *comp_sides);

#ifdef __cplusplus
}
#endif
#endif
