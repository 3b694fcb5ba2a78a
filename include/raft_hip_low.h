/* raft_hip_low.h -- where a read is NOT covered: the low-coverage runs of a finished pass, in libraft_hip_low.so.
 *
 * The entry points of raft_hip.h are a closed set (ABI 11).  This query ships beside them, in a library of its own built from the
 * same tree: it takes the context raft_hip_create made, after raft_hip_finish, and reads what the pass left on the device.
 * Link -lraft_hip_low -lraft_hip.  raft_hip_low_abi() returns the RAFT_HIP_ABI_VERSION the library was built beside; a caller
 * checks it against raft_hip_abi_version() once. */
#ifndef RAFT_HIP_LOW_H
#define RAFT_HIP_LOW_H
#include "raft_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

int raft_hip_low_abi(void);

/*  * The low-coverage runs of every read of the finished pass.  Window w of read r (cov_offset[r] <= w < cov_offset[r + 1]) is low
 * when cov[w] <= low_cov; window j = w - cov_offset[r] covers the bases [j * reso, min((j + 1) * reso, len[r])).  A run is a
 * maximal sequence of consecutive low windows j1..j2 of ONE read (it never continues into the next read's first window):
 *     low_s = j1 * reso,   low_e = min((j2 + 1) * reso, len[r])        (clamped directly: not the repeat scan's flanks)
 * Outputs, CSR in read order as rep_* is:
 *     low_offset[n_reads + 1]   runs of read r are low_offset[r] <= k < low_offset[r + 1]
 *     low_s[], low_e[]          [n_runs], ascending within a read
 *     low_windows[n_reads]      low windows of the read
 *     low_flags[n_reads]        RAFT_HIP_LOW_INTERIOR  some run has j1 > 0 and j2 < W - 1 (W = the read's windows): a chimera candidate
 *                               RAFT_HIP_LOW_HEAD      a run with j1 == 0
 *                               RAFT_HIP_LOW_TAIL      a run with j2 == W - 1 (a read that is one run end to end: HEAD | TAIL)
 *                               RAFT_HIP_LOW_UNCOVERED 1000 * low_bases[r] > uncovered_permille * len[r] in 64-bit integers,
 *                                                      low_bases[r] = sum of low_e - low_s over the read's runs
 * A read without windows has no run, 0 low windows and flags 0.  n_runs <= RAFT_HIP_LOW_RUNS_MAX(n_bins, n_reads) always: a
 * caller can size low_s / low_e from the pass's summary without a query.
 * All output arrays are host arrays; any may be NULL (it is then not copied), sum may be NULL.  low_s / low_e are copied only
 * when sum->n_runs <= run_cap; otherwise nothing of the two is copied, sum->n_runs says what is needed and the code is
 * RAFT_HIP_ERR_TOO_LARGE -- the conventions of raft_hip_fetch_packed.  The size query (low_s = low_e = NULL) always succeeds.
 * low_cov < 0 or uncovered_permille outside [0, 1000] -> RAFT_HIP_ERR_PARAM.  Valid exactly where raft_hip_read_stats is,
 * otherwise RAFT_HIP_ERR_STATE.  Like it, the call writes nothing of the pass, hands out no geometry, and reads the coverage in
 * the form the pass wrote: int32; one / two bytes per window read in place while low_cov lies below the code's limit (255 /
 * 65535: a code at the limit is then above low_cov whatever the listed value is); otherwise, and for four-bit steps, decoded into
 * int32 first.  A pass whose exception list is incomplete -> RAFT_HIP_ERR_DEVICE.  The stream is waited for twice: for the run
 * total, which sizes the run arrays on the device, and at the end.  kernel_seconds (may be NULL): device time of the launches. */
#define RAFT_HIP_LOW_INTERIOR  1
#define RAFT_HIP_LOW_HEAD      2
#define RAFT_HIP_LOW_TAIL      4
#define RAFT_HIP_LOW_UNCOVERED 8
#define RAFT_HIP_LOW_RUNS_MAX(n_bins, n_reads) (((int64_t)(n_bins) + (int64_t)(n_reads)) / 2)
typedef struct raft_hip_low_summary {
    int64_t n_runs;            /* runs of all reads */
    int64_t low_windows;       /* sum of low_windows[] */
    int64_t low_bases;         /* sum of low_e - low_s */
    int64_t reads_with_runs, reads_interior, reads_uncovered;   /* reads with a run / with RAFT_HIP_LOW_INTERIOR / with _UNCOVERED */
} raft_hip_low_summary;
int raft_hip_low_coverage(raft_hip_ctx *ctx, int32_t low_cov, int32_t uncovered_permille,
                          int64_t run_cap, int64_t *low_offset, int32_t *low_s, int32_t *low_e,
                          int32_t *low_windows, uint8_t *low_flags,
                          raft_hip_low_summary *sum, double *kernel_seconds);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
