// containment_lib.hip -- libraft_hip_ctn.so: raft_hip_containment_device / _host and raft_hip_place_contained_device / _host
// (include/raft_hip_ctn.h): the forest of the contained reads of a record stream, and that forest on a unitig layout.
//
// A library of its own beside libraft_hip.so (the others: the SIDE list of raft_amd/csrc/Makefile): the set of entry points of
// include/raft_hip.h is closed (ABI 11), and these calls need nothing of the engine but the context they are handed -- the stream, and
// buffers registered with the context like every other (ctn[...], and the queries' shared staging q_len, q_col).  They read no
// finished pass and leave the context's state as it is.
#include "query_host.hpp"
#include "../../include/raft_hip_ctn.h"
#include "containment.hpp"

namespace {

// the buffers of c->ctn
enum CtnBuf {
    kBufWork,        // key1, key2, tree_bases (64 bit), then flag words, children, tree_reads, tree_depth (32 bit): cleared as one
    kBufStateA, kBufStateB, kBufOut32, kBufFlags, kBufCtl, kBufStrand,
    kBufPlcUnitig, kBufPlcStart, kBufPlcOrient, kBufPlcAcc, kBufPlcDepth, kBufPlcCtl,
    kBufPlcFlags, kBufPlcOrientIn, kBufPlcWide,      // the host form's staging: flags, orient; offset and utg_length
    kBufCount
};
static_assert(kBufCount == kCtnBufs, "engine_ctx.hpp declares as many");
static_assert(RAFT_HIP_CTN_HAS_PARENT == kCtnHasParent && RAFT_HIP_CTN_PARENT_REV == kCtnParentRev && RAFT_HIP_CTN_ROOT_REV == kCtnRootRev &&
              RAFT_HIP_CTN_UNPLACED_VIEW == kCtnUnplacedView && RAFT_HIP_CTN_ORPHAN == kCtnOrphan && RAFT_HIP_CTN_MAX_READS == kCtnMaxReads,
              "the constants of the header");
static_assert(sizeof(raft::CtnState) == 16, "a state is one 16-byte line");

struct CtnCall {
    int32_t n_reads;
    const int32_t *len;
    RecordCols rec;
    const uint8_t *strand;
    int32_t max_overhang, min_ratio, symmetric;
    int32_t *parent, *pos, *span, *root, *root_pos, *depth, *children; uint8_t *flags; int32_t *tree_reads; int64_t *tree_bases; int32_t *tree_depth;
    raft_hip_ctn_summary *sum; int64_t *error_index; double *kernel_seconds;
};

constexpr const char *kWho = "containment";
constexpr const char *kWhoPlace = "place_contained";

// what both forms check before anything is staged
int check_call(raft_hip_ctx *c, const CtnCall &a)
{
    PHASE(check_ends_rule_call(c, kWho, a.max_overhang, a.min_ratio, a.n_reads, a.len, a.rec, a.strand));
    if (a.n_reads > kCtnMaxReads) return refuse(c, RAFT_HIP_ERR_TOO_LARGE, kWho, "n_reads is above 2^30 - 1");
    return RAFT_HIP_OK;
}

// the four-record loads: the six columns on 16-byte lines, strand on a 4-byte one
bool vector_path(const CtnCall &a)
{
    return aligned16(a.rec) && (reinterpret_cast<uintptr_t>(a.strand) & 3) == 0;
}

// a: device arrays but for the outputs
int ctn_run(raft_hip_ctx *c, const CtnCall &a)
{
    const int64_t n_rec = a.rec.n_rec;
    const size_t n = (size_t)std::max(a.n_reads, 1);
    HIP_TRY(c, c->ctn[kBufWork].ensure(n * (3 * 8 + 4 * 4)));
    HIP_TRY(c, c->ctn[kBufStateA].ensure(n * sizeof(CtnState)));
    HIP_TRY(c, c->ctn[kBufStateB].ensure(n * sizeof(CtnState)));
    HIP_TRY(c, c->ctn[kBufOut32].ensure(n * 6 * 4));
    HIP_TRY(c, c->ctn[kBufFlags].ensure(n));
    HIP_TRY(c, c->ctn[kBufCtl].ensure((size_t)kCtnCtlWords * 8));
    QueryTimer timer(c, a.kernel_seconds);
    if (a.kernel_seconds) *a.kernel_seconds = 0.0;
    unsigned long long *ctl = c->ctn[kBufCtl].as<unsigned long long>();
    unsigned long long *key1 = c->ctn[kBufWork].as<unsigned long long>(), *key2 = key1 + n, *bases = key1 + 2 * n;
    unsigned *flagw = reinterpret_cast<unsigned *>(key1 + 3 * n), *children = flagw + n;
    const CtnAcc acc{bases, flagw + 2 * n, flagw + 3 * n};
    CtnState *state[2] = {c->ctn[kBufStateA].as<CtnState>(), c->ctn[kBufStateB].as<CtnState>()};
    int32_t *out32 = c->ctn[kBufOut32].as<int32_t>();
    const CtnInitOut init_out{out32, out32 + n, out32 + 2 * n};
    const CtnEmitOut emit_out{out32 + 3 * n, out32 + 4 * n, out32 + 5 * n, c->ctn[kBufFlags].as<uint8_t>()};
    int64_t launches = 0;
    PHASE(clear_ctl(c, ctl, kCtnCtlWords));
    PHASE(timer.start());
    int last = 0;                            // which half holds the final states
    HIP_TRY(c, hipMemsetAsync(key1, 0, n * (3 * 8 + 4 * 4), c->stream));
    if (n_rec > 0) {                         // (without reads every id is out of range: pass 1 keeps record 0)
        const int32_t *const *col = a.rec.col;
        const CtnStreamArgs A{a.len, col[0], col[1], col[2], col[3], col[4], col[5], a.strand, (long long)n_rec, a.n_reads, a.max_overhang,
                              a.min_ratio, a.symmetric ? 1 : 0, key1, key2, flagw, ctl};
        const dim3 grid(stream_grid(n_rec)), block(kStreamThreads);
        if (vector_path(a)) {
            hipLaunchKernelGGL((ctn_stream_kernel<true, 1>), grid, block, 0, c->stream, A);
            hipLaunchKernelGGL((ctn_stream_kernel<true, 2>), grid, block, 0, c->stream, A);
        } else {
            hipLaunchKernelGGL((ctn_stream_kernel<false, 1>), grid, block, 0, c->stream, A);
            hipLaunchKernelGGL((ctn_stream_kernel<false, 2>), grid, block, 0, c->stream, A);
        }
        launches += 2;
    }
    if (a.n_reads > 0) {
        const dim3 grid(ctn_grid(a.n_reads)), block(kCtnThreads);
        hipLaunchKernelGGL(ctn_init_kernel, grid, block, 0, c->stream, a.n_reads, key1, key2, flagw, children, state[0], init_out);
        const int rounds = ctn_rounds(a.n_reads);
        for (int k = 0; k < rounds; ++k) {
            if (k + 1 < rounds) hipLaunchKernelGGL(ctn_jump_kernel<false>, grid, block, 0, c->stream, a.n_reads, a.len, state[last], state[last ^ 1], ctl);
            else hipLaunchKernelGGL(ctn_jump_kernel<true>, grid, block, 0, c->stream, a.n_reads, a.len, state[last], state[last ^ 1], ctl);
            last ^= 1;
        }
        hipLaunchKernelGGL(ctn_tree_kernel, dim3(stream_grid(a.n_reads)), dim3(kStreamThreads), 0, c->stream, state[last], a.len, a.n_reads, acc);
        hipLaunchKernelGGL(ctn_emit_kernel, grid, block, 0, c->stream, state[last], flagw, a.n_reads, acc, emit_out, ctl);
        launches += 3 + rounds;
    }
    HIP_TRY(c, hipGetLastError());
    PHASE(timer.stop());
    unsigned long long h_ctl[kCtnCtlWords] = {};
    PHASE(read_ctl(c, ctl, h_ctl, kCtnCtlWords));
    HIP_TRY(c, hipStreamSynchronize(c->stream));              // (the one wait for the control words: the first bad record, the open states, the totals)
    PHASE(timer.seconds(a.kernel_seconds));
    PHASE(first_bad_record(c, h_ctl[0], a.error_index, "containment: a record names a read id outside [0, n_reads)"));
    if (h_ctl[kCtnCtlOpen] != 0) {
        c->last_error = "containment: " + std::to_string(h_ctl[kCtnCtlOpen]) + " reads did not reach a root in ceil(log2(n_reads)) rounds";
        return RAFT_HIP_ERR_DEVICE;
    }
    const size_t n_reads = (size_t)a.n_reads;
    PHASE(queue_copies(c, {{a.parent, init_out.parent, n_reads * 4}, {a.pos, init_out.pos, n_reads * 4}, {a.span, init_out.span, n_reads * 4},
                           {a.root, emit_out.root, n_reads * 4}, {a.root_pos, emit_out.root_pos, n_reads * 4}, {a.depth, emit_out.depth, n_reads * 4},
                           {a.children, children, n_reads * 4}, {a.flags, emit_out.flags, n_reads}, {a.tree_reads, acc.reads, n_reads * 4},
                           {a.tree_bases, acc.bases, n_reads * 8}, {a.tree_depth, acc.depth, n_reads * 4}}));
    HIP_TRY(c, hipStreamSynchronize(c->stream));              // (... and the one for the copies)
    const unsigned long long *t = h_ctl + kCtnCtlTotals;
    if (a.sum)
        *a.sum = raft_hip_ctn_summary{n_rec, (int64_t)h_ctl[kCtnCtlViews], (int64_t)h_ctl[kCtnCtlNotLonger], (int64_t)t[kCtnWithParent],
                                      (int64_t)t[kCtnOrphans], (int64_t)t[kCtnRoots], (int64_t)t[kCtnRootsWithTree], (int64_t)t[kCtnGreatestDepth],
                                      (int64_t)t[kCtnLargestReads], (int64_t)t[kCtnLargestBases], launches};
    return RAFT_HIP_OK;
}

struct PlcCall {
    int32_t n_reads;
    const int32_t *len, *root, *root_pos; const uint8_t *flags; const int32_t *unitig; const int64_t *offset; const uint8_t *orient;
    int32_t n_unitigs; const int64_t *utg_length;
    int32_t *placed_unitig; int64_t *start; uint8_t *placed_orient; int32_t *placed_reads; int64_t *placed_bases, *depth_permille;
    raft_hip_place_summary *sum; int64_t *error_index; double *kernel_seconds;
};

int check_place(raft_hip_ctx *c, const PlcCall &a)
{
    if (!c) return RAFT_HIP_ERR_PARAM;
    if (a.n_reads < 0) return refuse(c, RAFT_HIP_ERR_PARAM, kWhoPlace, "n_reads is negative");
    if (a.n_unitigs < 0) return refuse(c, RAFT_HIP_ERR_PARAM, kWhoPlace, "n_unitigs is negative");
    if (a.n_reads > 0 && (!a.len || !a.root || !a.root_pos || !a.flags || !a.unitig || !a.offset || !a.orient))
        return refuse(c, RAFT_HIP_ERR_PARAM, kWhoPlace, "a missing array (read_len, root, root_pos, flags, unitig, offset, orient)");
    if (a.n_unitigs > 0 && !a.utg_length) return refuse(c, RAFT_HIP_ERR_PARAM, kWhoPlace, "utg_length is missing");
    if (a.n_reads > kCtnMaxReads) return refuse(c, RAFT_HIP_ERR_TOO_LARGE, kWhoPlace, "n_reads is above 2^30 - 1");
    return RAFT_HIP_OK;
}

int plc_run(raft_hip_ctx *c, const PlcCall &a)
{
    const size_t n = (size_t)std::max(a.n_reads, 1), U = (size_t)std::max(a.n_unitigs, 1);
    HIP_TRY(c, c->ctn[kBufPlcUnitig].ensure(n * 4));
    HIP_TRY(c, c->ctn[kBufPlcStart].ensure(n * 8));
    HIP_TRY(c, c->ctn[kBufPlcOrient].ensure(n));
    HIP_TRY(c, c->ctn[kBufPlcAcc].ensure(U * (8 + 4 + 4)));
    HIP_TRY(c, c->ctn[kBufPlcDepth].ensure(U * 8));
    HIP_TRY(c, c->ctn[kBufPlcCtl].ensure((size_t)kPlcCtlWords * 8));
    QueryTimer timer(c, a.kernel_seconds);
    if (a.kernel_seconds) *a.kernel_seconds = 0.0;
    unsigned long long *ctl = c->ctn[kBufPlcCtl].as<unsigned long long>();
    unsigned long long *bases = c->ctn[kBufPlcAcc].as<unsigned long long>();
    const PlcAcc acc{bases, reinterpret_cast<unsigned *>(bases + U), reinterpret_cast<unsigned *>(bases + U) + U};
    long long *depth = c->ctn[kBufPlcDepth].as<long long>();
    const PlcArgs A{a.n_reads, a.n_unitigs, a.len, a.root, a.root_pos, a.flags, a.unitig, reinterpret_cast<const long long *>(a.offset), a.orient,
                    c->ctn[kBufPlcUnitig].as<int32_t>(), c->ctn[kBufPlcStart].as<long long>(), c->ctn[kBufPlcOrient].as<uint8_t>(), acc, ctl};
    PHASE(clear_ctl(c, ctl, kPlcCtlWords));
    PHASE(timer.start());
    HIP_TRY(c, hipMemsetAsync(bases, 0, U * (8 + 4 + 4), c->stream));
    if (a.n_reads > 0) hipLaunchKernelGGL(ctn_place_kernel, dim3(stream_grid(a.n_reads)), dim3(kStreamThreads), 0, c->stream, A);
    if (a.n_unitigs > 0)
        hipLaunchKernelGGL(ctn_depth_kernel, dim3(ctn_grid(a.n_unitigs)), dim3(kCtnThreads), 0, c->stream, a.n_unitigs,
                           reinterpret_cast<const long long *>(a.utg_length), acc, depth, ctl);
    HIP_TRY(c, hipGetLastError());
    PHASE(timer.stop());
    unsigned long long h_ctl[kPlcCtlWords] = {};
    PHASE(read_ctl(c, ctl, h_ctl, kPlcCtlWords));
    HIP_TRY(c, hipStreamSynchronize(c->stream));              // (the one wait for the control words)
    PHASE(timer.seconds(a.kernel_seconds));
    PHASE(first_bad_record(c, h_ctl[0], a.error_index, "place_contained: a read names a unitig outside [-1, n_unitigs) or a root outside [0, n_reads)"));
    const size_t n_reads = (size_t)a.n_reads, n_utg = (size_t)a.n_unitigs;
    PHASE(queue_copies(c, {{a.placed_unitig, A.placed_unitig, n_reads * 4}, {a.start, A.start, n_reads * 8}, {a.placed_orient, A.placed_orient, n_reads},
                           {a.placed_reads, acc.reads, n_utg * 4}, {a.placed_bases, acc.bases, n_utg * 8}, {a.depth_permille, depth, n_utg * 8}}));
    HIP_TRY(c, hipStreamSynchronize(c->stream));              // (... and the one for the copies)
    if (a.sum)
        *a.sum = raft_hip_place_summary{(int64_t)a.n_reads, (int64_t)a.n_unitigs, (int64_t)h_ctl[kPlcCtlPlaced], (int64_t)a.n_reads - (int64_t)h_ctl[kPlcCtlPlaced],
                                        (int64_t)h_ctl[kPlcCtlGained], (int64_t)h_ctl[kPlcCtlGreatest]};
    return RAFT_HIP_OK;
}

} // namespace

extern "C" {

int raft_hip_ctn_abi(void) { return RAFT_HIP_ABI_VERSION; }

int raft_hip_containment_device(raft_hip_ctx *c, int32_t n_reads, const int32_t *d_read_len, int64_t n_rec, const int32_t *d_qid,
                                const int32_t *d_qs, const int32_t *d_qe, const int32_t *d_tid, const int32_t *d_ts, const int32_t *d_te,
                                const uint8_t *d_strand, int32_t max_overhang, int32_t min_ratio_permille, int32_t symmetric,
                                int32_t *parent, int32_t *pos, int32_t *span, int32_t *root, int32_t *root_pos, int32_t *depth,
                                int32_t *children, uint8_t *flags, int32_t *tree_reads, int64_t *tree_bases, int32_t *tree_depth,
                                raft_hip_ctn_summary *sum, int64_t *error_index, double *kernel_seconds)
{
    const CtnCall a{n_reads, d_read_len, {n_rec, {d_qid, d_qs, d_qe, d_tid, d_ts, d_te}}, d_strand, max_overhang, min_ratio_permille, symmetric,
                    parent, pos, span, root, root_pos, depth, children, flags, tree_reads, tree_bases, tree_depth, sum, error_index, kernel_seconds};
    PHASE(check_call(c, a));
    HIP_TRY(c, hipSetDevice(c->device));
    return ctn_run(c, a);
}

// The same from host arrays: the lengths and the six columns staged through q_len and q_col, which no pass uses, the strand bytes
// through a buffer of the set.
int raft_hip_containment_host(raft_hip_ctx *c, int32_t n_reads, const int32_t *read_len, int64_t n_rec, const int32_t *qid,
                              const int32_t *qs, const int32_t *qe, const int32_t *tid, const int32_t *ts, const int32_t *te,
                              const uint8_t *strand, int32_t max_overhang, int32_t min_ratio_permille, int32_t symmetric,
                              int32_t *parent, int32_t *pos, int32_t *span, int32_t *root, int32_t *root_pos, int32_t *depth,
                              int32_t *children, uint8_t *flags, int32_t *tree_reads, int64_t *tree_bases, int32_t *tree_depth,
                              raft_hip_ctn_summary *sum, int64_t *error_index, double *kernel_seconds)
{
    CtnCall a{n_reads, read_len, {n_rec, {qid, qs, qe, tid, ts, te}}, strand, max_overhang, min_ratio_permille, symmetric,
              parent, pos, span, root, root_pos, depth, children, flags, tree_reads, tree_bases, tree_depth, sum, error_index, kernel_seconds};
    PHASE(check_call(c, a));
    HIP_TRY(c, hipSetDevice(c->device));
    PHASE(stage_host(c, c->q_len, read_len, (size_t)n_reads, &a.len));
    if (n_rec > 0) {
        PHASE(stage_columns(c, c->q_col, a.rec));
        PHASE(stage_host(c, c->ctn[kBufStrand], strand, (size_t)n_rec, &a.strand));
    }
    return ctn_run(c, a);
}

int raft_hip_place_contained_device(raft_hip_ctx *c, int32_t n_reads, const int32_t *d_read_len, const int32_t *d_root,
                                    const int32_t *d_root_pos, const uint8_t *d_flags, const int32_t *d_unitig, const int64_t *d_offset,
                                    const uint8_t *d_orient, int32_t n_unitigs, const int64_t *d_utg_length, int32_t *placed_unitig,
                                    int64_t *start, uint8_t *placed_orient, int32_t *placed_reads, int64_t *placed_bases,
                                    int64_t *depth_permille, raft_hip_place_summary *sum, int64_t *error_index, double *kernel_seconds)
{
    const PlcCall a{n_reads, d_read_len, d_root, d_root_pos, d_flags, d_unitig, d_offset, d_orient, n_unitigs, d_utg_length,
                    placed_unitig, start, placed_orient, placed_reads, placed_bases, depth_permille, sum, error_index, kernel_seconds};
    PHASE(check_place(c, a));
    HIP_TRY(c, hipSetDevice(c->device));
    return plc_run(c, a);
}

// The same from host arrays: the lengths through q_len, root, root_pos and unitig through q_col[0 .. 2], the rest through buffers of
// the set (offset and utg_length share one: offset [n_reads], then utg_length).
int raft_hip_place_contained_host(raft_hip_ctx *c, int32_t n_reads, const int32_t *read_len, const int32_t *root,
                                  const int32_t *root_pos, const uint8_t *flags, const int32_t *unitig, const int64_t *offset,
                                  const uint8_t *orient, int32_t n_unitigs, const int64_t *utg_length, int32_t *placed_unitig,
                                  int64_t *start, uint8_t *placed_orient, int32_t *placed_reads, int64_t *placed_bases,
                                  int64_t *depth_permille, raft_hip_place_summary *sum, int64_t *error_index, double *kernel_seconds)
{
    PlcCall a{n_reads, read_len, root, root_pos, flags, unitig, offset, orient, n_unitigs, utg_length,
              placed_unitig, start, placed_orient, placed_reads, placed_bases, depth_permille, sum, error_index, kernel_seconds};
    PHASE(check_place(c, a));
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = (size_t)n_reads, U = (size_t)n_unitigs;
    PHASE(stage_host(c, c->q_len, read_len, n, &a.len));
    PHASE(stage_host(c, c->q_col[0], root, n, &a.root));
    PHASE(stage_host(c, c->q_col[1], root_pos, n, &a.root_pos));
    PHASE(stage_host(c, c->q_col[2], unitig, n, &a.unitig));
    PHASE(stage_host(c, c->ctn[kBufPlcFlags], flags, n, &a.flags));
    PHASE(stage_host(c, c->ctn[kBufPlcOrientIn], orient, n, &a.orient));
    HIP_TRY(c, c->ctn[kBufPlcWide].ensure((n + U + 1) * 8));
    int64_t *wide = c->ctn[kBufPlcWide].as<int64_t>();
    if (n > 0) HIP_TRY(c, hipMemcpyAsync(wide, offset, n * 8, hipMemcpyHostToDevice, c->stream));
    if (U > 0) HIP_TRY(c, hipMemcpyAsync(wide + n, utg_length, U * 8, hipMemcpyHostToDevice, c->stream));
    a.offset = wide; a.utg_length = wide + n;
    return plc_run(c, a);
}

} // extern "C"
