/* raft_host_utg.h -- the host text layer's part of `raft --unitigs`: the writer of PREFIX.unitigs.tsv and
 * PREFIX.unitigs.layout.tsv (libraft_host.so, beside the functions of raft_host.h). */
#ifndef RAFT_HOST_UTG_H
#define RAFT_HOST_UTG_H
#include "raft_host.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Two files, no header line, tab-separated, from raft_hip_unitigs_*'s outputs (include/raft_hip_utg.h) for the reads of `reads`:
 *     PREFIX.unitigs.tsv         one line per unitig in id order:     unitig  reads  length  circular  first_read  last_read
 *     PREFIX.unitigs.layout.tsv  one line per read in layout order:   unitig  index  name  length  orient  offset
 * first_read and last_read are the names of the first and the last read of the layout, circular is 0 or 1, orient '+' or '-',
 * length in the second file the read's.  SKIPPED reads (unitig -1) do not appear.  n_unitigs is U; the per-read arrays are
 * [n_reads], order [utg_off[U]], utg_off [U + 1], the per-unitig arrays [U].  A table that names a read outside the set, or whose
 * offsets do not ascend from 0, is refused (RAFT_HOST_ERR_ARG) before anything is written. */
int raft_host_write_unitigs(const char *prefix, const raft_host_reads *reads, int64_t n_unitigs, const int32_t *unitig, const int32_t *index,
                            const int64_t *offset, const uint8_t *orient, const int32_t *order, const int64_t *utg_off,
                            const int32_t *utg_reads, const int64_t *utg_length, const uint8_t *utg_circular);

#ifdef __cplusplus
}
#endif
#endif
