/* raft_host_sg.h -- the host text layer's part of `raft --string-graph`: the writer of PREFIX.string_graph.gfa and
 * PREFIX.string_graph.tsv (libraft_host.so, beside the functions of raft_host.h). */
#ifndef RAFT_HOST_SG_H
#define RAFT_HOST_SG_H
#include "raft_host.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Two files from raft_hip_string_graph_*'s outputs (include/raft_hip_sg.h) for the reads of `reads`:
 *     PREFIX.string_graph.gfa   H\tVN:Z:1.0, then one  S\tname\t*\tLN:i:length  per read that is not flagged (flags without
 *                               RAFT_HIP_BEST_SKIPPED) in read order, then one  L\ta\t[+-]\tb\t[+-]\t<span>M  per edge in list order:
 *                               a is the read of edge_u and '+' when the edge leaves its 3' end, b the read of edge_w and '+' when
 *                               the edge enters its 5' end
 *     PREFIX.string_graph.tsv   one line per read in read order, tab-separated, no header:  name  length  arcs5  kept5  arcs3  kept3
 * arcs and kept are [2 * n_reads], flags [n_reads], the three edge arrays [n_edges] (the list as the caller wants it drawn: the
 * surviving edges, or with emit_removed all of them).  A list that names a node outside [0, 2 * n_reads) or an end of a flagged read
 * is refused (RAFT_HOST_ERR_ARG) before anything is written.  The bytes do not depend on the number of threads. */
int raft_host_write_string_graph(const char *prefix, const raft_host_reads *reads, const int32_t *arcs, const int32_t *kept, const uint8_t *flags,
                                 int64_t n_edges, const int32_t *edge_u, const int32_t *edge_w, const int32_t *edge_span);

#ifdef __cplusplus
}
#endif
#endif
