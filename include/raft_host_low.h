/* raft_host_low.h -- the host text layer's writer for `raft --low-cov` (libraft_host.so, beside the functions of raft_host.h). */
#ifndef RAFT_HOST_LOW_H
#define RAFT_HOST_LOW_H
#include "raft_host.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The low-coverage runs of `raft --low-cov` (PREFIX.low_coverage.bed): one line per run, "name\tstart\tend\tclass\n", in read
 * order and ascending by start within a read.  low_offset / low_s / low_e as raft_hip_low_coverage gives them (include/raft_hip_low.h);
 * class is "whole" (the run begins at base 0 and ends at the read's length), "head" (begins at 0), "tail" (ends at the length)
 * or "interior".  reso is the window size the runs were made under (> 0). */
int raft_host_write_low_coverage(const char *path, int32_t n_reads, const char *const *names, const int64_t *low_offset,
                                 const int32_t *low_s, const int32_t *low_e, const int32_t *read_len, int32_t reso);

#ifdef __cplusplus
}
#endif
#endif
