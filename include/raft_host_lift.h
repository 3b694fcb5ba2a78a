/* raft_host_lift.h -- the host text layer's part of `raft --fragment-paf`: the writer of PREFIX.fragments.paf (libraft_host.so,
 * beside the functions of raft_host.h). */
#ifndef RAFT_HOST_LIFT_H
#define RAFT_HOST_LIFT_H
#include "raft_host.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One 12-field PAF line per output of raft_hip_lift_overlaps_* (include/raft_hip_lift.h), in their order, for the reads of `reads`
 * and the fragment table the outputs were lifted against:
 *     qname  qlen  qs  qe  strand  tname  tlen  ts  te  matches  block  255
 * A fragment's name is exactly the first word of its header in PREFIX.reads.fasta as raft_host_write_fasta writes it for the same
 * table -- ">read=<row + 1>,..." without the '>' up to the first blank, in both header forms (real and simulated reads; both
 * writers take the header from one helper) -- and "read=<row + 1>" for a fragment that file gives no header.  A fragment's length
 * is fe - fb of its row; strand is '-' where rev != 0.
 *   matches == NULL (block is then not looked at): field 11 is the larger of the two spans, field 10 the smaller.
 *   otherwise matches and block are PAF fields 10 and 11 of the stream the outputs were lifted from, indexed by src (which must then
 *   be there): field 11 is the larger span B, field 10 is min(B, floor(matches[src] * B / block[src])), and 0 when block[src] <= 0
 *   (a negative matches[src] counts as 0).
 * Lines are formatted by the layer's worker threads and written in order: the bytes do not depend on the thread count.  A row
 * outside [0, n_frag) is refused (RAFT_HOST_ERR_ARG) before anything is written. */
int raft_host_write_fragment_paf(const char *path, const raft_host_reads *reads, const int64_t *frag_offset, const int32_t *frag_begin,
                                 const int32_t *frag_end, int64_t n_out, const int32_t *qfrag, const int32_t *qs, const int32_t *qe,
                                 const int32_t *tfrag, const int32_t *ts, const int32_t *te, const uint8_t *rev, const int32_t *src,
                                 const int32_t *matches, const int32_t *block);

#ifdef __cplusplus
}
#endif
#endif
