/* raft_host_frag.h -- the host text layer's writer for `raft --fragment-overlaps` (libraft_host.so, beside the functions of raft_host.h). */
#ifndef RAFT_HOST_FRAG_H
#define RAFT_HOST_FRAG_H
#include "raft_host.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The table of `raft --fragment-overlaps` (PREFIX.fragments.tsv), from the fragment rows and what raft_hip_frag_overlaps_* gives
 * (include/raft_hip_frag.h).  Tab-separated, no header line, names as they are; one line per fragment in row order,
 *       read_num  name  begin  end  touching  spanning  contained  repeat_bases
 *   read_num = the row index + 1: the number in the fragment's FASTA header (">read=<read_num>,..."); name = the name of the read
 *   the row belongs to; begin / end = frag_begin / frag_end; touching / spanning / contained = frag_touch / frag_span /
 *   frag_contained; repeat_bases = frag_repeat.
 * frag_offset [n_reads + 1] must begin at 0 and not descend (otherwise RAFT_HOST_ERR_ARG, nothing written).  The lines are formatted
 * by the layer's worker threads in blocks of reads and written in order: the bytes do not depend on the number of threads. */
int raft_host_write_fragments(const char *path, int32_t n_reads, const char *const *names, const int64_t *frag_offset,
                              const int32_t *frag_begin, const int32_t *frag_end, const int32_t *frag_touch, const int32_t *frag_span,
                              const int32_t *frag_contained, const int32_t *frag_repeat);

#ifdef __cplusplus
}
#endif
#endif
