/* raft_host_cln.h -- the host text layer's part of `raft --graph-clean`: the writer of PREFIX.clean.tsv (libraft_host.so, beside the
 * functions of raft_host.h).  The cleaned graph itself and its unitigs are written by raft_host_write_string_graph and
 * raft_host_write_unitigs under the prefix PREFIX.clean. */
#ifndef RAFT_HOST_CLN_H
#define RAFT_HOST_CLN_H
#include "raft_host.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One file, no header line, tab-separated, one line per read in read order, from raft_hip_graph_clean_*'s outputs
 * (include/raft_hip_cln.h) for the reads of `reads`:
 *     name length state round weak5 kept5 weak3 kept3
 * state is `kept`, `tip` or `flagged` (read_state 0, 1, 2), round the round in which a tip was removed (else 0); weak5 / kept5 and
 * weak3 / kept3 are the arcs the weak cut removed and the live degree at the read's 5' and 3' end.  read_state and read_round are
 * [n_reads], weak and kept [2 * n_reads].  A read_state above 2 or a negative count is refused (RAFT_HOST_ERR_ARG) before anything is
 * written.  The bytes do not depend on the number of threads. */
int raft_host_write_graph_clean(const char *path, const raft_host_reads *reads, const uint8_t *read_state, const uint8_t *read_round,
                                const int32_t *weak, const int32_t *kept);

#ifdef __cplusplus
}
#endif
#endif
