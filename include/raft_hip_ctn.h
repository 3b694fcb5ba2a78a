/* raft_hip_ctn.h -- the containment forest: in which read every contained read sits, where, on which strand, and through how many
 * containers it reaches a read that stays; and, in a second call, the forest laid onto the unitigs of raft_hip_utg.h, so that a
 * layout holds every read and not its backbone alone.  In libraft_hip_ctn.so.
 *
 * The entry points of raft_hip.h are a closed set (ABI 11).  These calls ship beside them, in a library of its own built from the
 * same tree, as raft_hip_sg.h and the eleven before it do: they take the context raft_hip_create made.  Link -lraft_hip_ctn
 * -lraft_hip.  raft_hip_ctn_abi() returns the RAFT_HIP_ABI_VERSION the library was built beside; a caller checks it against
 * raft_hip_abi_version() once.  They look at no finished pass and are valid in any state of the context, which they leave as it is (a
 * pass in flight on the stream is waited for). */
#ifndef RAFT_HIP_CTN_H
#define RAFT_HIP_CTN_H
#include "raft_hip_end.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

int raft_hip_ctn_abi(void);

/*  * The rule (integers only).  Records, lengths, strand, H = max_overhang and F = min_ratio_permille are those of raft_hip_end.h, and
 * so is a record's kind.
 *
 * Views.  A containment view is a record of kind QUERY_CONTAINED seen from its query: r = qid, c = tid, [as, ae) = [qs, qe),
 * [bs, be) = [ts, te).  Unless symmetric != 0 a record of kind TARGET_CONTAINED also gives a view from its target, with the roles
 * swapped.  A record and its mirror give the same views.  With lr = len[r], lc = len[c] the view is ACCEPTABLE iff
 * lc > lr or (lc == lr and c < r): the ends rule lets a longer read lie inside a shorter one when the two aligned spans differ in
 * length, and acceptability is what makes the parent relation a strict order -- the result is a forest, never a cycle.  Every other
 * containment view is counted (views_not_longer) and flags r with RAFT_HIP_CTN_UNPLACED_VIEW; it adds nothing else.
 *
 * Parent.  key1 = (uint64)lc << 31 | (uint64)(0x7FFFFFFF - c).  The parent of r is the c of the greatest key1 over r's acceptable
 * views: the longest container, then the smaller id.  0 means no parent.
 *
 * Place in the parent.  Over the acceptable views of r whose c is that parent: span = min(ae - as, be - bs);
 * pos_raw = rev ? bs - (lr - ae) : bs - as; pos = min(max(pos_raw, 0), lc - lr);
 * key2 = (uint64)span << 32 | (uint64)rev << 31 | (uint64)(0x7FFFFFFF - pos).  The greatest key2 wins: the longest span, then '-'
 * before '+' as raft_hip_best.h has it, then the smaller pos.  Equal keys are indistinguishable in the output, so the table is a
 * function of the multiset of records, not of their order and not of scheduling.
 *
 * To the root.  A read without a parent is a root: root = r, root_pos = 0, root_rev = 0, depth = 0.  Otherwise, with parent a at
 * (p, v) and a in its root at (P, V): root_pos(r) = V ? P + (len[a] - p - lr) : P + p; root_rev = v ^ V; depth = depth(a) + 1.  By
 * the clamp 0 <= root_pos <= len[root] - lr always holds: nothing is an error in a coordinate. */
#define RAFT_HIP_CTN_HAS_PARENT 1
#define RAFT_HIP_CTN_PARENT_REV 2      /* the read lies reversed in its parent */
#define RAFT_HIP_CTN_ROOT_REV 4        /* ... in its root */
#define RAFT_HIP_CTN_UNPLACED_VIEW 8   /* some containment view of the read is not acceptable */
#define RAFT_HIP_CTN_ORPHAN 16         /* UNPLACED_VIEW without HAS_PARENT: some view contains the read, no view places it */
#define RAFT_HIP_CTN_MAX_READS 1073741823      /* 2^30 - 1 */

/*  * Per read, [n_reads] each: parent (int32, -1 for none), pos and span (int32, 0 without a parent); root, root_pos, depth (int32);
 * children (int32: the reads whose parent it is); flags (uint8, the bits above).  Per root, in the rows of the root reads and 0
 * elsewhere: tree_reads (int32) and tree_bases (int64), the reads below the root and their summed lengths, and tree_depth (int32),
 * the deepest read below it.
 *
 * raft_hip_ctn_summary: records = n_rec; containment_views; views_not_longer; reads_with_parent; orphans; roots; roots_with_tree
 * (tree_reads > 0); greatest_depth; largest_tree_reads and largest_tree_bases (not necessarily of the same tree); launches, the
 * number of kernels the call launched.
 *
 * _device: read_len, the six columns and strand (uint8 [n_rec]) are DEVICE arrays.  _host: they are host arrays, staged by the
 * library.  Every output is host memory in both forms and may be NULL, the summary, error_index and kernel_seconds (the device time
 * of the launches, from events on the context's stream) included.
 *
 * A record whose qid or tid lies outside [0, n_reads) is RAFT_HIP_ERR_READ_ID, with the smallest index of such a record in
 * *error_index; no output but error_index and kernel_seconds is then written.  Without such a record *error_index is -1.
 *
 * Refused before any launch, with a message (raft_hip_last_error) that starts "containment:": with RAFT_HIP_ERR_PARAM what
 * raft_hip_overlap_ends_* refuses -- max_overhang < 0, min_ratio_permille outside [0, 1000], n_reads < 0, n_rec < 0, read_len missing
 * while n_reads > 0, with n_rec > 0 a missing column (the six and strand) --, with RAFT_HIP_ERR_TOO_LARGE n_reads > 2^30 - 1.
 * n_rec == 0 and n_reads == 0 are valid: every read a root. */
typedef struct raft_hip_ctn_summary {
    int64_t records;
    int64_t containment_views;
    int64_t views_not_longer;
    int64_t reads_with_parent;
    int64_t orphans;
    int64_t roots;
    int64_t roots_with_tree;
    int64_t greatest_depth;
    int64_t largest_tree_reads;
    int64_t largest_tree_bases;
    int64_t launches;
} raft_hip_ctn_summary;

int raft_hip_containment_device(raft_hip_ctx *ctx, int32_t n_reads, const int32_t *d_read_len, int64_t n_rec, const int32_t *d_qid,
                                const int32_t *d_qs, const int32_t *d_qe, const int32_t *d_tid, const int32_t *d_ts, const int32_t *d_te,
                                const uint8_t *d_strand, int32_t max_overhang, int32_t min_ratio_permille, int32_t symmetric,
                                int32_t *parent, int32_t *pos, int32_t *span, int32_t *root, int32_t *root_pos, int32_t *depth,
                                int32_t *children, uint8_t *flags, int32_t *tree_reads, int64_t *tree_bases, int32_t *tree_depth,
                                raft_hip_ctn_summary *sum, int64_t *error_index, double *kernel_seconds);
int raft_hip_containment_host(raft_hip_ctx *ctx, int32_t n_reads, const int32_t *read_len, int64_t n_rec, const int32_t *qid,
                              const int32_t *qs, const int32_t *qe, const int32_t *tid, const int32_t *ts, const int32_t *te,
                              const uint8_t *strand, int32_t max_overhang, int32_t min_ratio_permille, int32_t symmetric,
                              int32_t *parent, int32_t *pos, int32_t *span, int32_t *root, int32_t *root_pos, int32_t *depth,
                              int32_t *children, uint8_t *flags, int32_t *tree_reads, int64_t *tree_bases, int32_t *tree_depth,
                              raft_hip_ctn_summary *sum, int64_t *error_index, double *kernel_seconds);

/*  * Second call: the forest on a layout.  The inputs are read_len, the forest's root, root_pos and flags (of which ROOT_REV is read),
 * the per-read outputs of raft_hip_unitigs_*: unitig (int32), offset (int64) and orient (uint8), and n_unitigs with utg_length
 * (int64 [n_unitigs]).  The table is not trusted: a unitig outside [-1, n_unitigs) or a root outside [0, n_reads) returns
 * RAFT_HIP_ERR_READ_ID with the smallest such read in *error_index, and no output is written; otherwise *error_index is -1.
 *
 * For read r with root R in unitig u >= 0 at (off, o): placed_unitig = u; start = o ? off + (len[R] - root_pos - lr) : off + root_pos
 * (int64); placed_orient = o ^ root_rev.  A root is placed at its own offset.  A read whose root has unitig -1 (an orphan's tree, a
 * read left out) is unplaced: -1, 0, 0.  There is NO WRAP on circular unitigs: a read placed near the end of a cycle's layout may
 * reach beyond its length.
 *
 * Per unitig, [n_unitigs] each: placed_reads (int32, the backbone included), placed_bases (int64, the summed lengths; a length below
 * 0 counts as 0) and depth_permille (int64) = placed_bases * 1000 / length, 0 when length == 0.
 *
 * raft_hip_place_summary: n_reads; n_unitigs; placed; unplaced; unitigs_gained, the unitigs that hold a read with a parent;
 * greatest_depth_permille.
 *
 * _device: every input array is a DEVICE array.  _host: host arrays, staged by the library.  Every output is host memory in both
 * forms and may be NULL.  Refused with RAFT_HIP_ERR_PARAM before any launch, with a message that starts "place_contained:":
 * n_reads < 0, n_unitigs < 0, an input per read missing while n_reads > 0, utg_length missing while n_unitigs > 0; with
 * RAFT_HIP_ERR_TOO_LARGE n_reads > 2^30 - 1.  n_reads == 0 and n_unitigs == 0 are valid. */
typedef struct raft_hip_place_summary {
    int64_t n_reads;
    int64_t n_unitigs;
    int64_t placed;
    int64_t unplaced;
    int64_t unitigs_gained;
    int64_t greatest_depth_permille;
} raft_hip_place_summary;

int raft_hip_place_contained_device(raft_hip_ctx *ctx, int32_t n_reads, const int32_t *d_read_len, const int32_t *d_root,
                                    const int32_t *d_root_pos, const uint8_t *d_flags, const int32_t *d_unitig, const int64_t *d_offset,
                                    const uint8_t *d_orient, int32_t n_unitigs, const int64_t *d_utg_length, int32_t *placed_unitig,
                                    int64_t *start, uint8_t *placed_orient, int32_t *placed_reads, int64_t *placed_bases,
                                    int64_t *depth_permille, raft_hip_place_summary *sum, int64_t *error_index, double *kernel_seconds);
int raft_hip_place_contained_host(raft_hip_ctx *ctx, int32_t n_reads, const int32_t *read_len, const int32_t *root,
                                  const int32_t *root_pos, const uint8_t *flags, const int32_t *unitig, const int64_t *offset,
                                  const uint8_t *orient, int32_t n_unitigs, const int64_t *utg_length, int32_t *placed_unitig,
                                  int64_t *start, uint8_t *placed_orient, int32_t *placed_reads, int64_t *placed_bases,
                                  int64_t *depth_permille, raft_hip_place_summary *sum, int64_t *error_index, double *kernel_seconds);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
