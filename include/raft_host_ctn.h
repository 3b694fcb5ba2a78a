/* raft_host_ctn.h -- the host text layer's part of `raft --containment`: the writers of PREFIX.containment.tsv and
 * PREFIX.unitigs.depth.tsv (libraft_host.so, beside the functions of raft_host.h). */
#ifndef RAFT_HOST_CTN_H
#define RAFT_HOST_CTN_H
#include "raft_host.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One file, no header line, tab-separated, one line per read in read order, from raft_hip_containment_*'s outputs and, where they are
 * given, raft_hip_place_contained_*'s (include/raft_hip_ctn.h) for the reads of `reads`:
 *     name length parent strand pos span root root_strand root_pos depth children tree_reads tree_bases placed_unitig start orient
 * parent and root are names; strand, root_strand and orient are '+' or '-' (bits PARENT_REV and ROOT_REV of flags; placed_orient).  A
 * read without a parent has `* * 0 0` for parent, strand, pos and span.  A read that is not placed (placed_unitig -1), and every read
 * when placed_unitig, start and placed_orient are NULL (all three or none), has `* 0 *` for the last three.  All arrays are [n_reads].
 * A table that names a parent outside [-1, n_reads), a root outside [0, n_reads) or a unitig below -1 is refused
 * (RAFT_HOST_ERR_ARG) before anything is written.  The bytes do not depend on the number of threads. */
int raft_host_write_containment(const char *path, const raft_host_reads *reads, const int32_t *parent, const int32_t *pos, const int32_t *span,
                                const int32_t *root, const int32_t *root_pos, const int32_t *depth, const int32_t *children, const uint8_t *flags,
                                const int32_t *tree_reads, const int64_t *tree_bases, const int32_t *placed_unitig, const int64_t *start,
                                const uint8_t *placed_orient);

/* One file, no header line, tab-separated, one line per unitig in id order, from raft_hip_unitigs_*'s utg_reads and utg_length and
 * raft_hip_place_contained_*'s per-unitig outputs, [n_unitigs] each:
 *     unitig reads length placed_reads placed_bases depth_permille */
int raft_host_write_unitig_depth(const char *path, int64_t n_unitigs, const int32_t *utg_reads, const int64_t *utg_length, const int32_t *placed_reads,
                                 const int64_t *placed_bases, const int64_t *depth_permille);

#ifdef __cplusplus
}
#endif
#endif
