/* raft_hip_rst.h -- one row per repeat run: how deep it is piled, how many overlap sides reach into it, lie wholly inside it, and cover
 * it end to end, in libraft_hip_rst.so.
 *
 * The entry points of raft_hip.h are a closed set (ABI 11).  This query ships beside them, in a library of its own built from the
 * same tree, as raft_hip_low.h, raft_hip_ovl.h and raft_hip_frag.h do: it takes the context raft_hip_create made.  Link
 * -lraft_hip_rst -lraft_hip.  raft_hip_rst_abi() returns the RAFT_HIP_ABI_VERSION the library was built beside; a caller checks it
 * against raft_hip_abi_version() once. */
#ifndef RAFT_HIP_RST_H
#define RAFT_HIP_RST_H
#include "raft_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

int raft_hip_rst_abi(void);

/*  * Runs.  The annotation is rep_offset int64 [n_reads + 1], rep_s / rep_e int32 [n_rep]; run k of read r
 * (rep_offset[r] <= k < rep_offset[r + 1]) is the half-open interval [s, e) = [rep_s[k], rep_e[k]).  Within a read rep_s is
 * non-decreasing (the walk below relies on it); rep_e need not be: flanks make neighbouring runs overlap, and runs clamped to
 * start 0 tie on rep_s in no particular order (raft_hip_ovl.h).  Every output here is PER RUN, never on the union of a read's runs.
 * Coordinates are taken as they are: nothing is clipped to the read's length and no coordinate is an error.  len = read_len[r].
 *
 * run_flags[k] (uint8):
 *     RAFT_HIP_RST_EMPTY     e <= s
 *     RAFT_HIP_RST_AT_START  s <= 0
 *     RAFT_HIP_RST_AT_END    e >= len
 * The three bits are independent.  A run with no bit is interior: it has a real flank on both sides.
 *
 * Counted sides, exactly as intervals[] of raft_hip_census_* counts them: the query side [qs, qe) of every record with qid == r
 * and, when symmetric == 0, the target side [ts, te) of every record with tid == r && tid != qid.  ts / te may be NULL only when
 * symmetric != 0.  `records` NULL or n_rec == 0: no records, every count is 0.
 * A side [a, b) with b <= a counts nothing, and an EMPTY run is counted by nothing.  Otherwise, for run [s, e):
 *     run_touch[k]   counts the sides with a < e && b > s
 *     run_span[k]    counts the sides with a <= s && b >= e      (the side covers the run end to end)
 *     run_inside[k]  counts the sides with a >= s && b <= e      (the side may exist only because of the run)
 * A side equal to the run is all three; a spanning or an inside side touches.  All three are int32.  On the device touch and span
 * of a run are the two halves of ONE 64-bit word that only ever receives positive adds: the halves lie 32 bits apart and do not mix
 * below 2^32 sides on a run, and n_rec < 2^30 (below) keeps every run under 2^31.
 *
 * Coverage part, when threshold >= 1.  The call reads the coverage of the context's finished pass: it is valid exactly where
 * raft_hip_read_stats is (otherwise RAFT_HIP_ERR_STATE) and n_reads must be that pass's (otherwise RAFT_HIP_ERR_PARAM) -- with an
 * explicit annotation too.  W = the read's windows in that pass, reso its window size.  In 64 bits
 *     j0 = max(s, 0) / reso,  j1 = min(ceil(e / reso), W),  run_windows[k] = max(j1 - j0, 0), and 0 for an EMPTY run;
 *     run_cov_sum (int64), run_cov_min, run_cov_max, run_high (int32: windows with cov >= threshold) are taken over the windows
 *     j0 .. j1 - 1 of the read; all four are 0 when there are none.
 * int32 coverage is read in place; any other form the pass holds (one or two bytes plus the exception list, four-bit steps) is
 * decoded into int32 first, into a buffer of this query's.  An incomplete exception list is RAFT_HIP_ERR_DEVICE.  Nothing of the
 * pass is written and no geometry is handed out (a later speculated pass still reports RAFT_HIP_SUM_KEPT_GEOMETRY).
 * threshold == 0: no coverage part; the five coverage outputs must be NULL (RAFT_HIP_ERR_PARAM otherwise); with an explicit
 * annotation the call is then valid in any state of the context (a pass in flight on the stream is waited for).
 * threshold < 0 -> RAFT_HIP_ERR_PARAM.
 *
 * The annotation is an argument with exactly the conventions of raft_hip_repeat_overlaps_*: all three arrays NULL with
 * n_rep == -1 is the context's own finished pass (valid where raft_hip_read_stats is, n_reads must be that pass's; the outputs
 * then have summary.n_repeats rows); explicit arrays are DEVICE arrays in the _device form and host arrays in the _host form; with
 * n_rep == 0 rep_s / rep_e may be NULL.  The kernel that walks the reads checks rep_offset[0] == 0,
 * rep_offset[r] <= rep_offset[r + 1] and rep_offset[n_reads] == n_rep: a violation is RAFT_HIP_ERR_PARAM, and the record kernel
 * reads no record and no run (every workgroup leaves at its first instruction).
 *
 * Errors.  An id outside [0, n_reads) -> RAFT_HIP_ERR_READ_ID with *error_index the first such record (either column); otherwise
 * *error_index = -1.  n_rec >= 2^30 or n_rep >= 2^31 - 1 -> RAFT_HIP_ERR_TOO_LARGE.  A missing column, a negative count (other
 * than the -1 above) -> RAFT_HIP_ERR_PARAM.  Results reach the caller's arrays only when the call succeeds.
 *
 * Outputs: the nine arrays [n_rep] and the summary are HOST memory in both forms; any of them may be NULL.  read_len and the
 * record columns are device arrays in the _device form and host arrays in the _host form, which stages its arguments through
 * buffers of the context that no pass uses, as raft_hip_census_host does.  kernel_seconds (may be NULL): device time of the
 * launches, from events on the context's stream. */
#define RAFT_HIP_RST_EMPTY    1
#define RAFT_HIP_RST_AT_START 2
#define RAFT_HIP_RST_AT_END   4
typedef struct raft_hip_rst_summary {
    int64_t n_runs;
    int64_t runs_empty;                                /* RAFT_HIP_RST_EMPTY */
    int64_t runs_interior;                             /* run_flags == 0 */
    int64_t runs_touched;                              /* run_touch > 0 */
    int64_t runs_spanned;                              /* run_span > 0 */
    int64_t interior_spanned;                          /* run_flags == 0 && run_span > 0 */
    int64_t sides_touch, sides_span, sides_inside;     /* the sums of the three count arrays */
    int64_t windows;                                   /* the sum of run_windows (0 without the coverage part) */
    int64_t cov_sum;                                   /* the sum of run_cov_sum */
} raft_hip_rst_summary;

/* `records` is raft_hip_records of raft_hip.h: n_rec and the six columns (DEVICE arrays in the _device form, host arrays in the _host form). */
int raft_hip_repeat_stats_device(raft_hip_ctx *ctx, int32_t n_reads, const int32_t *d_read_len, const raft_hip_records *records,
                                 int32_t symmetric, int64_t n_rep, const int64_t *d_rep_offset, const int32_t *d_rep_s,
                                 const int32_t *d_rep_e, int32_t threshold,
                                 int32_t *run_touch, int32_t *run_span, int32_t *run_inside,
                                 int32_t *run_windows, int32_t *run_cov_min, int32_t *run_cov_max, int32_t *run_high,
                                 int64_t *run_cov_sum, uint8_t *run_flags,
                                 raft_hip_rst_summary *sum, int64_t *error_index, double *kernel_seconds);
int raft_hip_repeat_stats_host(raft_hip_ctx *ctx, int32_t n_reads, const int32_t *read_len, const raft_hip_records *records,
                               int32_t symmetric, int64_t n_rep, const int64_t *rep_offset, const int32_t *rep_s,
                               const int32_t *rep_e, int32_t threshold,
                               int32_t *run_touch, int32_t *run_span, int32_t *run_inside,
                               int32_t *run_windows, int32_t *run_cov_min, int32_t *run_cov_max, int32_t *run_high,
                               int64_t *run_cov_sum, uint8_t *run_flags,
                               raft_hip_rst_summary *sum, int64_t *error_index, double *kernel_seconds);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
