/* raft_hip_frag.h -- which fragments stay contained: the record stream joined with the fragment table, in libraft_hip_frag.so.
 *
 * The entry points of raft_hip.h are a closed set (ABI 11).  This query ships beside them, in a library of its own built from the
 * same tree, as raft_hip_low.h and raft_hip_ovl.h do: it takes the context raft_hip_create made.  Link -lraft_hip_frag -lraft_hip.
 * raft_hip_frag_abi() returns the RAFT_HIP_ABI_VERSION the library was built beside; a caller checks it against
 * raft_hip_abi_version() once. */
#ifndef RAFT_HIP_FRAG_H
#define RAFT_HIP_FRAG_H
#include "raft_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

int raft_hip_frag_abi(void);

/*  * The fragment table.  frag_offset is int64 [n_reads + 1], frag_begin (fb) and frag_end (fe) are int32 [n_frag]; row k is the
 * half-open interval [fb[k], fe[k]); F(r) are the rows frag_offset[r] <= k < frag_offset[r + 1].  A read may have no rows.  The device
 * checks all of
 *     frag_offset[0] == 0, frag_offset[r] <= frag_offset[r + 1], frag_offset[n_reads] == n_frag;
 *     within a read fb does not descend and fe does not descend;
 *     0 <= fb[k] <= fe[k];
 * a violation is RAFT_HIP_ERR_PARAM, and the record kernel then reads no record and no row (every workgroup leaves at its first
 * instruction).  The engine's own fragments satisfy this (both bounds strictly ascend within a read).
 *
 * Counted sides.  A record with qid == tid contributes nothing.  Otherwise its query side [qs, qe) on read qid is counted with
 * partner side [ts, te) on read tid and, when symmetric == 0, its target side [ts, te) on read tid is counted with the query side
 * as partner.  Coordinates are taken as they are: nothing is clipped and no coordinate is an error.  A side with b <= a contributes
 * nothing.  All six columns are required whenever n_rec > 0, under either value of `symmetric`: the partner check needs them.
 *
 * One counted side [a, b) on read r with partner side [c, d) on read p (every comparison in 64 bits):
 *     row k of F(r) is TOUCHED    when fe[k] > a && fb[k] < b
 *     row k of F(r) is SPANNED    when fb[k] >= a && fe[k] <= b, and it is touched
 *     the partner is WHOLE        when d > c and some row g of F(p) has fb[g] <= c && d <= fe[g]
 *     row k is CONTAINED by the side when it is spanned and the partner is whole: the fragment's image lies inside ONE fragment of
 *                                 the partner, so an assembler sees the fragment as contained again.
 * No length comparison is made: this is the weak, sufficient rule -- whoever is spanned end to end by an overlap whose other side
 * was left in one piece counts, whichever of the two is longer.  A partner side that crosses one of the partner's cuts decides
 * nothing: the row is spanned, not contained.
 *
 * Outputs.
 *   per fragment, int32 [n_frag]:
 *     frag_touch, frag_span, frag_contained   the number of counted sides with that property
 *     frag_repeat[k] = |[fb[k], fe[k]) intersected with U(r)|, U(r) the SET UNION of the read's repeat runs exactly as raft_hip_ovl.h
 *                      defines it (rep_s non-decreasing within a read, rep_e not necessarily)
 *   per read, int32 [n_reads]:
 *     read_contained[r]   the rows of F(r) with frag_contained > 0
 *   raft_hip_frag_summary (below).
 * The per-fragment arrays are the caller's DEVICE arrays in the _device form and host arrays in the _host form; read_contained and
 * the summary are host memory in both.  Any output may be NULL.
 *
 * The table and the annotation are arguments, a small struct each (never NULL themselves).
 *   raft_hip_frag_table: explicit arrays (device arrays in the _device form, host arrays in the _host form) may be passed in any state
 *     of the context; a pass in flight on the stream is waited for.  With n_frag == 0 frag_begin / frag_end may be NULL.  All three
 *     NULL with n_frag == -1: the context's own finished pass -- valid exactly where raft_hip_read_stats is (otherwise
 *     RAFT_HIP_ERR_STATE); n_reads must be that pass's (otherwise RAFT_HIP_ERR_PARAM); nothing of the pass is written and no geometry
 *     is handed out (a later speculated pass still reports RAFT_HIP_SUM_KEPT_GEOMETRY).  The own table is whole behind a pass run
 *     with raft_hip_set_emit_cuts(ctx, 0) too: only the cut points (cuts[]) wait for the first fetch that asks for them, every pass
 *     writes its frag_* rows and rep_* runs itself, and this call neither needs nor materialises the cut points.
 *   raft_hip_frag_repeats: as in raft_hip_repeat_overlaps_*: explicit arrays (rep_offset int64 [n_reads + 1], rep_s / rep_e int32
 *     [n_rep]; checked as there, a violation is RAFT_HIP_ERR_PARAM), or all NULL with n_rep == -1 for the context's own finished pass
 *     (the same state rule), or all NULL with n_rep == 0 for none: frag_repeat is then all zeros.
 *   Only some of the three arrays of either NULL (but for the row arrays of an empty table or annotation) -> RAFT_HIP_ERR_PARAM.
 *
 * Errors.  An id outside [0, n_reads) -> RAFT_HIP_ERR_READ_ID with *error_index the first such record (within one record the query
 * column is looked at first); otherwise *error_index = -1.  n_rec >= 2^30 or n_frag >= 2^31 - 1 -> RAFT_HIP_ERR_TOO_LARGE (the
 * counters are int32: 2^30 records have 2^31 sides).  A missing column, a negative count (other than the -1 above) ->
 * RAFT_HIP_ERR_PARAM.  No output is written on any error.
 *
 * The _host form stages its arguments through buffers of the context that no pass uses, as raft_hip_census_host does.
 * kernel_seconds (may be NULL): device time of the launches, from events on the context's stream. */
typedef struct raft_hip_frag_table {
    int64_t n_frag;                                    /* rows; -1 with the arrays NULL: the context's own finished pass */
    const int64_t *frag_offset;                        /* [n_reads + 1] */
    const int32_t *frag_begin, *frag_end;              /* [n_frag] */
} raft_hip_frag_table;
typedef struct raft_hip_frag_repeats {
    int64_t n_rep;                                     /* runs; -1 with the arrays NULL: the context's own pass; 0 with them NULL: none */
    const int64_t *rep_offset;                         /* [n_reads + 1] */
    const int32_t *rep_s, *rep_e;                      /* [n_rep] */
} raft_hip_frag_repeats;
typedef struct raft_hip_frag_summary {
    int64_t n_records;
    int64_t n_fragments;
    int64_t frags_untouched;                           /* rows with frag_touch == 0 */
    int64_t frags_spanned;                             /* frag_span > 0 */
    int64_t frags_contained;                           /* frag_contained > 0 */
    int64_t frags_contained_repeat;                    /* frag_contained > 0 and frag_repeat > 0 */
    int64_t reads_whole_spanned;                       /* some counted side of the read has a <= 0 && b >= len[r]: the same rule before fragmentation */
    int64_t reads_any_contained;                       /* read_contained > 0 */
    int64_t reads_all_contained;                       /* reads with at least one row whose every row is contained */
} raft_hip_frag_summary;

/* `records` is raft_hip_records of raft_hip.h: n_rec and the six columns (DEVICE arrays in the _device form, host arrays in the _host form). */
int raft_hip_frag_overlaps_device(raft_hip_ctx *ctx, int32_t n_reads, const int32_t *d_read_len, const raft_hip_records *records,
                                  int32_t symmetric, const raft_hip_frag_table *table, const raft_hip_frag_repeats *repeats,
                                  int32_t *d_frag_touch, int32_t *d_frag_span, int32_t *d_frag_contained, int32_t *d_frag_repeat,
                                  int32_t *read_contained, raft_hip_frag_summary *sum, int64_t *error_index, double *kernel_seconds);
int raft_hip_frag_overlaps_host(raft_hip_ctx *ctx, int32_t n_reads, const int32_t *read_len, const raft_hip_records *records,
                                int32_t symmetric, const raft_hip_frag_table *table, const raft_hip_frag_repeats *repeats,
                                int32_t *frag_touch, int32_t *frag_span, int32_t *frag_contained, int32_t *frag_repeat,
                                int32_t *read_contained, raft_hip_frag_summary *sum, int64_t *error_index, double *kernel_seconds);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
