/* raft_hip_utg.h -- the unitigs of the best overlap graph: the chains and cycles that the mutual best overlaps of
 * raft_hip_best_overlaps_* form, the order, orientation and offset of every read in them, their lengths, in libraft_hip_utg.so.
 *
 * The entry points of raft_hip.h are a closed set (ABI 11).  This call ships beside them, in a library of its own built from the
 * same tree, as raft_hip_best.h and the six before it do: it takes the context raft_hip_create made.  Link -lraft_hip_utg
 * -lraft_hip.  raft_hip_utg_abi() returns the RAFT_HIP_ABI_VERSION the library was built beside; a caller checks it against
 * raft_hip_abi_version() once.  It looks at no finished pass and is valid in any state of the context, which it leaves as it is (a
 * pass in flight on the stream is waited for). */
#ifndef RAFT_HIP_UTG_H
#define RAFT_HIP_UTG_H
#include "raft_hip_best.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

int raft_hip_utg_abi(void);

/*  * The rule (integers only).  The input is n_reads, read_len (int32 [n_reads], a length below 0 counts as 0) and the three outputs of
 * raft_hip_best_overlaps_*: partner (int32 [2 * n_reads], index 2 * r + E), span (int32 [2 * n_reads]) and flags (uint8 [n_reads],
 * the bits RAFT_HIP_BEST_*).  Only an end with its MUTUAL bit is an edge; partner and span of any other end are not looked at.
 *
 * Half-edges.  h = 2 * r + E is "the walk leaves read r through end E" (0 = 5', 1 = 3').  twin(h) = h ^ 1.  If end (r, E) is mutual
 * with partner p on strand rev, then E' = rev ? E : 1 - E (the partner's end, raft_hip_best.h) and succ(h) = 2 * p + (1 - E'): the
 * walk enters p at E' and leaves it at the other end.  Otherwise succ(h) = NIL.  The step has the weight w(h) = len(p) - span(r, E).
 *
 * Consistency.  The table is not trusted.  For every read r and end E with the MUTUAL bit: r is not SKIPPED; p = partner[2 * r + E]
 * lies in [0, n_reads) and p != r; p is not SKIPPED; p's flag byte has MUTUAL at E' and its REV bit at E' equals rev;
 * partner[2 * p + E'] == r; span[2 * r + E] == span[2 * p + E']; 1 <= span <= min(len(r), len(p)).  An end that violates this makes
 * the call return RAFT_HIP_ERR_READ_ID with the smallest read id that has such an end in *error_index, and no output is written.
 * Otherwise *error_index is -1.  What raft_hip_best_overlaps_* writes always passes: a flagged read is no candidate on either side
 * and so has no best overlap at all; a key's partner is the other read of a record with two valid ids that is no self overlap (a
 * dovetail kind); MUTUAL is set exactly when the partner's slot holds a key that leads back to (r, E), and both keys then come from
 * views of overlaps between the same two reads at the same two ends, whose strand the ends determine (E' == E iff rev) and whose
 * span the greatest key of either side determines: were the spans different, the longer one would be a candidate of both slots
 * and beat the shorter one in the slot that holds it (with symmetric != 0 this needs what that flag promises, a stream that holds
 * every record's mirror).  A valid record has 1 <= span <= both lengths.
 *
 * Under the rule succ is injective (h = succ(g) names g through the partner slot of h's twin end), and because p != r no directed
 * path or cycle holds both h and twin(h); so every unitig is exactly two mirror-image directed components, both paths or both cycles.
 *
 * Unitigs.  A unitig is a connected component over the reads that are not SKIPPED; a read without a mutual end is a unitig of one
 * read.  Start and direction: a path of k >= 2 reads starts at the terminal read with the smaller id and is walked away from its
 * free end; k == 1 is the read itself, oriented '+'; a cycle starts at its smallest read id M, leaving through M's 3' end (M is '+'),
 * and is opened at the edge that enters 2 * M + 1.  Per read: orient is 0 ('+') if the walk from the start enters the read at its 5'
 * end, else 1; index is the number of reads before it; offset (int64) is the sum over the reads u before it of
 * len(u) - span(u -> next).  Per unitig: n_reads, circular, and length (int64): offset(last) + len(last) for a path, and for a
 * cycle the sum over all its reads u of len(u) - span(u -> next), the closing edge included.  Unitig ids are dense, 0 .. U - 1, in
 * the order of the start reads' ids.  The table is CSR like the repeat tables: utg_off (int64 [U + 1]) and order (int32 [reads in
 * unitigs]), the reads of unitig u in layout order at order[utg_off[u] .. utg_off[u + 1]).  SKIPPED reads have unitig -1, index -1,
 * offset 0, orient 0 and appear nowhere in order. */

/*  * raft_hip_utg_summary: reads_in = n_reads; reads_skipped the SKIPPED reads; unitigs = U; singletons the unitigs of one read;
 * circular the cycles; longest_reads and longest_length the greatest n_reads and the greatest length of a unitig (not necessarily
 * the same one); total_length the sum of all lengths.
 *
 * _device: read_len, partner, span and flags are DEVICE arrays (any 4-byte alignment; flags any).  _host: they are host arrays,
 * staged by the library.  Every output is host memory in both forms and may be NULL: per read unitig (int32), index (int32), offset
 * (int64), orient (uint8), each [n_reads]; order (int32 [n_reads]); utg_off (int64 [n_reads + 1]); per unitig utg_reads (int32),
 * utg_length (int64), utg_circular (uint8), each [n_reads].  There are at most n_reads unitigs and the call writes U (+ 1) entries
 * of the per-unitig arrays and n_reads - reads_skipped entries of order, so a caller that sizes them by n_reads (utg_off by
 * n_reads + 1) never has to ask twice; what lies behind is left as it was.  kernel_seconds is the device time of the launches,
 * from events on the context's stream; launches the number of kernels the call launched (the second ranking, which runs only
 * if the table holds a cycle, shows there: rounds + 2 more).
 *
 * Refused before any launch, with a message (raft_hip_last_error) that starts "unitigs:": n_reads < 0, or read_len, partner, span
 * or flags missing while n_reads > 0 (RAFT_HIP_ERR_PARAM); n_reads > 2^30 - 1 (RAFT_HIP_ERR_TOO_LARGE: half-edge ids are int32).
 * n_reads == 0 is valid: U = 0, utg_off[0] = 0. */
typedef struct raft_hip_utg_summary {
    int64_t reads_in;
    int64_t reads_skipped;
    int64_t unitigs;
    int64_t singletons;
    int64_t circular;
    int64_t longest_reads;
    int64_t longest_length;
    int64_t total_length;
} raft_hip_utg_summary;

int raft_hip_unitigs_device(raft_hip_ctx *ctx, int32_t n_reads, const int32_t *d_read_len, const int32_t *d_partner, const int32_t *d_span,
                            const uint8_t *d_flags, int32_t *unitig, int32_t *index, int64_t *offset, uint8_t *orient, int32_t *order,
                            int64_t *utg_off, int32_t *utg_reads, int64_t *utg_length, uint8_t *utg_circular, raft_hip_utg_summary *sum,
                            int64_t *error_index, double *kernel_seconds, int64_t *launches);
int raft_hip_unitigs_host(raft_hip_ctx *ctx, int32_t n_reads, const int32_t *read_len, const int32_t *partner, const int32_t *span,
                          const uint8_t *flags, int32_t *unitig, int32_t *index, int64_t *offset, uint8_t *orient, int32_t *order,
                          int64_t *utg_off, int32_t *utg_reads, int64_t *utg_length, uint8_t *utg_circular, raft_hip_utg_summary *sum,
                          int64_t *error_index, double *kernel_seconds, int64_t *launches);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
