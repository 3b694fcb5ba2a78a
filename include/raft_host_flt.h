/* raft_host_flt.h -- the host text layer's part of `raft --min-identity / --min-overlap`: a PAF tokenised WITH its columns 10 and 11
 * (libraft_host.so, beside the functions of raft_host.h).  The filter writes no file of its own: there is no writer here. */
#ifndef RAFT_HOST_FLT_H
#define RAFT_HOST_FLT_H
#include "raft_host.h"

#ifdef __cplusplus
extern "C" {
#endif

/* raft_host_paf_parse / raft_host_paf_load (raft_host.h) that also keep PAF field 10 (residue matches) and field 11 (alignment block
 * length) as two more int32 columns, under the numeric rules of the coordinates (plain digits, strtol's rules for anything else:
 * a field that is no number is 0, ten digits wrap as the coordinates do).  A line of exactly ten fields is a record, as it is for
 * the reference (paf.hpp:84): its block length is 0, so it fails every minimum identity above 0.  Field 11 ends at the next tab or
 * at the line's end, before a carriage return.  The six columns, the record count and the symmetric flag are exactly those of the
 * plain parser; names are resolved while tokenising, so a line that names an unknown read is RAFT_HOST_ERR_UNKNOWN_NAME whether a
 * filter would have dropped it or not. */
int raft_host_paf_parse_quality(raft_host_text *text, const raft_host_reads *reads, raft_host_paf **out, char *err_name, int err_cap);
int raft_host_paf_load_quality(const char *path, const raft_host_reads *reads, raft_host_paf **out, char *err_name, int err_cap);

/* k = 0: matches, k = 1: block; [raft_host_paf_count].  NULL for an object parsed without the columns, and for any other k. */
const int32_t *raft_host_paf_quality(const raft_host_paf *p, int k);

#ifdef __cplusplus
}
#endif
#endif
