/* raft_host_end.h -- the host text layer's part of `raft --overlap-ends`: a PAF tokenised WITH its strand (field 5), and the writer of
 * PREFIX.overlap_ends.tsv (libraft_host.so, beside the functions of raft_host.h). */
#ifndef RAFT_HOST_END_H
#define RAFT_HOST_END_H
#include "raft_host.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Which columns the tokeniser keeps beside the six: a bit mask. */
#define RAFT_HOST_PAF_QUALITY 1   /* fields 10 and 11 as raft_host_paf_parse_quality keeps them (raft_host_flt.h) */
#define RAFT_HOST_PAF_STRAND 2    /* field 5 as one byte per record */

/* raft_host_paf_parse / raft_host_paf_load (raft_host.h) that also keep the columns `columns` names.  The six columns, the record
 * count, the symmetric flag and the error behaviour are exactly those of the plain parser under every mask; columns = 0 is the
 * plain parser, columns = RAFT_HOST_PAF_QUALITY is raft_host_paf_parse_quality.  A bit other than the two is RAFT_HOST_ERR_ARG. */
int raft_host_paf_parse_with(raft_host_text *text, const raft_host_reads *reads, int columns, raft_host_paf **out, char *err_name, int err_cap);
int raft_host_paf_load_with(const char *path, const raft_host_reads *reads, int columns, raft_host_paf **out, char *err_name, int err_cap);

/* One byte per record [raft_host_paf_count]: 1 iff field 5 begins with '-' (the reference's rule, paf.hpp:69), else 0 -- '+', '*',
 * an empty field and anything else.  NULL for an object parsed without the column.  (raft_host_paf_quality of raft_host_flt.h gives
 * the quality columns of an object parsed with RAFT_HOST_PAF_QUALITY set.) */
const uint8_t *raft_host_paf_strand(const raft_host_paf *p);

/* PREFIX.overlap_ends.tsv: one line per read in read order, no header, tab-separated:
 *     name  length  internal  contained_in  contains  end5  end3  status
 * counts is raft_hip_overlap_ends_*'s table (int32 [5 * n_reads], counts[k * n_reads + r]), status its status bytes (as a number 0..4). */
int raft_host_write_overlap_ends(const char *path, const raft_host_reads *reads, const int32_t *counts, const uint8_t *status);

#ifdef __cplusplus
}
#endif
#endif
