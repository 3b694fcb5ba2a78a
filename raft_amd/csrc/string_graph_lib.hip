// string_graph_lib.hip -- libraft_hip_sg.so: raft_hip_string_graph_device / _host (include/raft_hip_sg.h), the string graph of a record
// stream: one arc per pair of read ends among the dovetails between the reads that are not left out, transitively reduced.
//
// A library of its own beside libraft_hip.so (the others: the SIDE list of raft_amd/csrc/Makefile): the set of entry points of
// include/raft_hip.h is closed (ABI 11), and this call needs nothing of the engine but the context it is handed -- the stream, and
// buffers registered with the context like every other (sg[], and the queries' shared staging q_len, q_col).  It reads no finished
// pass and leaves the context's state as it is.
//
// The call waits twice: once behind the count and its scan, for the number of views that give an arc -- it sizes the sort's buffers
// and grids, as n_out sizes lift_overlaps' outputs -- and once behind the last launch, where the control words are read.
#include "query_host.hpp"
#include "../../include/raft_hip_sg.h"
#include "device_scan.hpp"
#include "sort_pairs.hpp"
#include "string_graph.hpp"

namespace {

// the context's sg[] by name
enum SgBuf {
    kDig, kMask, kStepCnt, kStepOff, kItemU, kItemW, kItemExt, kItemBack, kItemSpan, kKeyA, kKeyB, kValA, kValB, kSortTmp, kHead, kChosen, kHeadPos,
    kArcU, kArcW, kArcExt, kArcBack, kArcSpan, kRow, kRed, kState, kEdgePos, kNodeArcs, kNodeKept, kNodeSole, kPartner, kSpan, kFlags,
    kEdgeU, kEdgeW, kEdgeSpan, kEdgeExt, kEdgeBack, kEdgeFlags, kCtl, kStage, kSgBufCount
};
static_assert(kSgBufCount == kSgBufs, "engine_ctx.hpp's count of this library's buffers");

struct SgCall {
    int32_t n_reads;
    const int32_t *len;
    RecordCols rec;
    const uint8_t *strand, *skip;
    int32_t max_overhang, min_ratio, symmetric, fuzz, emit_removed; int64_t out_cap;
    int32_t *arcs, *kept, *partner, *span; uint8_t *flags;
    int32_t *edge_u, *edge_w, *edge_span, *edge_ext, *edge_back; uint8_t *edge_flags; int64_t *n_out;
    raft_hip_sg_summary *sum; int64_t *error_index; double *kernel_seconds; int64_t *launches;
};

constexpr const char *kWho = "string_graph";
static_assert(RAFT_HIP_SG_EDGE_RED_U == kSgRedFromU && RAFT_HIP_SG_EDGE_RED_W == kSgRedFromW && RAFT_HIP_SG_EDGE_UNPAIRED == kSgUnpaired &&
              kSgStRed == kSgRedFromU && kSgStTwinRed == kSgRedFromW && kSgStUnpaired == kSgUnpaired, "the edge flags of the header");

// what both forms check before anything is staged
int check_call(raft_hip_ctx *c, const SgCall &a)
{
    PHASE(check_ends_rule_call(c, kWho, a.max_overhang, a.min_ratio, a.n_reads, a.len, a.rec, a.strand));
    if (a.fuzz < 0) return refuse(c, RAFT_HIP_ERR_PARAM, kWho, "fuzz is negative");
    if (a.out_cap < 0) return refuse(c, RAFT_HIP_ERR_PARAM, kWho, "out_cap is negative");
    if (a.n_reads > (int32_t(1) << 30) - 1 || a.rec.n_rec >= (int64_t(1) << 30))
        return refuse(c, RAFT_HIP_ERR_TOO_LARGE, kWho, "more than 2^30 - 1 reads or 2^30 records or more: nodes and views are int32");
    return RAFT_HIP_OK;
}

// the four-record loads: the six columns on 16-byte lines, strand on a 4-byte one
bool vector_path(const SgCall &a) { return aligned16(a.rec) && (reinterpret_cast<uintptr_t>(a.strand) & 3) == 0; }

int bits_for(long long n_values)
{
    int bits = 1;
    while (bits < 32 && (1ll << bits) < n_values) bits += 1;
    return bits;
}

// a: device arrays but for the outputs
int sg_run(raft_hip_ctx *c, const SgCall &a)
{
    const int64_t n_rec = a.rec.n_rec;
    const size_t n = (size_t)std::max(a.n_reads, 1);
    const long long n_nodes = 2ll * a.n_reads;
    const long long groups = sg_groups(n_rec), steps = sg_steps(n_rec);
    auto &B = c->sg;
    HIP_TRY(c, B[kDig].ensure(n * 4));
    HIP_TRY(c, B[kMask].ensure((size_t)std::max<long long>(groups, 1)));
    HIP_TRY(c, B[kStepCnt].ensure((size_t)std::max<long long>(steps, 1) * 4));
    HIP_TRY(c, B[kStepOff].ensure(((size_t)steps + 1 + (size_t)std::max(scan_blocks(steps), 1) + 1) * 8));
    HIP_TRY(c, B[kRow].ensure((2 * n + 1) * 4));
    for (int k : {kNodeArcs, kNodeKept, kNodeSole, kPartner, kSpan}) HIP_TRY(c, B[k].ensure(2 * n * 4));
    HIP_TRY(c, B[kFlags].ensure(n));
    HIP_TRY(c, B[kCtl].ensure((size_t)kSgCtlWords * 8));
    QueryTimer timer(c, a.kernel_seconds);
    double seconds[2] = {0.0, 0.0};
    if (a.kernel_seconds) *a.kernel_seconds = 0.0;
    if (a.launches) *a.launches = 0;
    unsigned long long *ctl = B[kCtl].as<unsigned long long>();
    unsigned *dig = B[kDig].as<unsigned>();
    long long *step_off = B[kStepOff].as<long long>();
    long long launches = 0;
    unsigned long long h_ctl[kSgCtlWords] = {};
    long long n_items = 0;

    // 1. the views that give an arc: a bit per view, a count per wave step, the steps' offsets
    PHASE(clear_ctl(c, ctl, kSgCtlWords));
    PHASE(timer.start());
    if (a.n_reads > 0) {
        hipLaunchKernelGGL(best_digest_kernel, dim3(grid_for(a.n_reads, 256, 1024)), dim3(256), 0, c->stream, a.len, a.skip, a.n_reads, dig);
        launches += 1;
    }
    const int32_t *const *col = a.rec.col;
    const SgStreamArgs A{dig, col[0], col[1], col[2], col[3], col[4], col[5], a.strand, (long long)n_rec, a.n_reads, a.max_overhang, a.min_ratio,
                         a.symmetric ? 1 : 0, B[kMask].as<uint8_t>(), B[kStepCnt].as<int32_t>(), ctl};
    const bool vec = vector_path(a);
    if (n_rec > 0) {
        const dim3 grid(stream_grid(n_rec)), block(kStreamThreads);
        if (vec) hipLaunchKernelGGL(sg_count_kernel<true>, grid, block, 0, c->stream, A);
        else hipLaunchKernelGGL(sg_count_kernel<false>, grid, block, 0, c->stream, A);
        exclusive_scan<SgStepLoader, 1>(c->stream, SgStepLoader{B[kStepCnt].as<int32_t>()}, steps, step_off + steps + 1, ScanOut<1>{{step_off}});
        launches += 3;
    }
    HIP_TRY(c, hipGetLastError());
    PHASE(timer.stop());
    PHASE(read_ctl(c, ctl, h_ctl, 1));
    if (n_rec > 0) PHASE(queue_copies(c, {{&n_items, step_off + steps, 8}}));
    HIP_TRY(c, hipStreamSynchronize(c->stream));              // (the first wait: the number of items sizes what follows)
    PHASE(timer.seconds(&seconds[0]));
    if (a.kernel_seconds) *a.kernel_seconds = seconds[0];
    if (a.launches) *a.launches = launches;
    PHASE(first_bad_record(c, h_ctl[0], a.error_index, "string_graph: a record names a read id outside [0, n_reads)"));
    if (n_items < 0 || n_items > 2 * n_rec) {
        c->last_error = "string_graph: the steps' offsets are out of range";
        return RAFT_HIP_ERR_DEVICE;
    }

    const size_t m = (size_t)std::max<long long>(n_items, 1);
    for (int k : {kItemU, kItemW, kItemExt, kItemBack, kItemSpan, kKeyA, kKeyB, kValA, kValB, kChosen, kArcU, kArcW, kArcExt, kArcBack, kArcSpan,
                  kEdgeU, kEdgeW, kEdgeSpan, kEdgeExt, kEdgeBack})
        HIP_TRY(c, B[k].ensure(m * 4));
    for (int k : {kHead, kRed, kState, kEdgeFlags}) HIP_TRY(c, B[k].ensure(m));
    HIP_TRY(c, B[kSortTmp].ensure(rs_tmp_bytes<int32_t>(n_items)));
    const size_t scan_words = m + 1 + (size_t)std::max(scan_blocks(n_items), 1) + 1;
    HIP_TRY(c, B[kHeadPos].ensure(scan_words * 8));
    HIP_TRY(c, B[kEdgePos].ensure(scan_words * 8));
    const SgItems items{B[kItemU].as<int32_t>(), B[kItemW].as<int32_t>(), B[kItemExt].as<int32_t>(), B[kItemBack].as<int32_t>(), B[kItemSpan].as<int32_t>(),
                        B[kKeyA].as<uint32_t>(), B[kValA].as<int32_t>(), n_items};
    const SgArcs arcs{B[kArcU].as<int32_t>(), B[kArcW].as<int32_t>(), B[kArcExt].as<int32_t>(), B[kArcBack].as<int32_t>(), B[kArcSpan].as<int32_t>()};
    const SgEdges edges{B[kEdgeU].as<int32_t>(), B[kEdgeW].as<int32_t>(), B[kEdgeSpan].as<int32_t>(), B[kEdgeExt].as<int32_t>(), B[kEdgeBack].as<int32_t>(),
                        B[kEdgeFlags].as<uint8_t>()};
    long long *head_pos = B[kHeadPos].as<long long>(), *edge_pos = B[kEdgePos].as<long long>();
    const long long *n_arcs_p = head_pos + n_items;          // the head scan's total
    int32_t *row = B[kRow].as<int32_t>();
    uint8_t *red = B[kRed].as<uint8_t>(), *state = B[kState].as<uint8_t>();
    const dim3 block(kSgThreads);
    long long n_arcs = 0, n_listed = 0;

    PHASE(timer.start());
    if (n_items > 0) {
        const dim3 igrid(sg_grid(n_items));
        {
            const dim3 grid(stream_grid(n_rec)), sblock(kStreamThreads);
            if (vec) hipLaunchKernelGGL(sg_fill_kernel<true>, grid, sblock, 0, c->stream, A, step_off, items);
            else hipLaunchKernelGGL(sg_fill_kernel<false>, grid, sblock, 0, c->stream, A, step_off, items);
            launches += 1;
        }
        // 2. by w, then (stable) by u
        const int bits = bits_for(n_nodes);
        uint32_t *key[2] = {B[kKeyA].as<uint32_t>(), B[kKeyB].as<uint32_t>()};
        int32_t *val[2] = {B[kValA].as<int32_t>(), B[kValB].as<int32_t>()};
        bool in_b = false;
        HIP_TRY(c, radix_sort_by_key<int32_t>(c->stream, key[0], val[0], key[1], val[1], n_items, bits, B[kSortTmp].p, &in_b, &launches));
        int at = in_b ? 1 : 0;
        hipLaunchKernelGGL(sg_rekey_kernel, igrid, block, 0, c->stream, val[at], items.u, n_items, key[at]);
        HIP_TRY(c, radix_sort_by_key<int32_t>(c->stream, key[at], val[at], key[1 - at], val[1 - at], n_items, bits, B[kSortTmp].p, &in_b, &launches));
        if (in_b) at = 1 - at;
        launches += 1;                                         // (the sorts add their own)
        // 3. one arc per (u, w), the rows
        hipLaunchKernelGGL(sg_choose_kernel, igrid, block, 0, c->stream, key[at], val[at], items, B[kHead].as<uint8_t>(), B[kChosen].as<int32_t>());
        exclusive_scan<SgByteLoader, 1>(c->stream, SgByteLoader{B[kHead].as<uint8_t>(), 1u}, n_items, head_pos + n_items + 1, ScanOut<1>{{head_pos}});
        hipLaunchKernelGGL(sg_compact_kernel, igrid, block, 0, c->stream, key[at], B[kHead].as<uint8_t>(), B[kChosen].as<int32_t>(), head_pos, items, arcs);
        hipLaunchKernelGGL(sg_rows_kernel, dim3(sg_grid(n_nodes + 1)), block, 0, c->stream, arcs.u, n_arcs_p, n_nodes, row);
        launches += 5;
        // 4. the reducible arcs
        HIP_TRY(c, hipMemsetAsync(red, 0, (size_t)n_items, c->stream));
        HIP_TRY(c, hipMemsetAsync(state, 0, (size_t)n_items, c->stream));
        hipLaunchKernelGGL(sg_reduce_kernel, dim3(grid_for(n_nodes, kWave, 1 << 16)), dim3(kWave), 0, c->stream, row, arcs.w, arcs.ext, n_nodes, a.fuzz, red);
        // 5. the twins, the survivors
        hipLaunchKernelGGL(sg_pair_kernel, igrid, block, 0, c->stream, row, arcs, n_arcs_p, red, a.emit_removed ? 1 : 0, state, ctl);
        launches += 2;
    } else {
        HIP_TRY(c, hipMemsetAsync(row, 0, (2 * n + 1) * 4, c->stream));
    }
    if (a.n_reads > 0) {
        hipLaunchKernelGGL(sg_ends_kernel, dim3(sg_grid(n_nodes)), block, 0, c->stream, row, state, n_nodes, B[kNodeArcs].as<int32_t>(), B[kNodeKept].as<int32_t>(),
                           B[kNodeSole].as<int32_t>());
        hipLaunchKernelGGL(sg_table_kernel, dim3(sg_grid(a.n_reads)), block, 0, c->stream, dig, a.n_reads, arcs, state, B[kNodeArcs].as<int32_t>(),
                           B[kNodeKept].as<int32_t>(), B[kNodeSole].as<int32_t>(), B[kPartner].as<int32_t>(), B[kSpan].as<int32_t>(), B[kFlags].as<uint8_t>(), ctl);
        launches += 2;
    }
    if (n_items > 0) {
        // (state is 0 behind the last arc: nothing is listed there)
        exclusive_scan<SgByteLoader, 1>(c->stream, SgByteLoader{state, kSgStListed}, n_items, edge_pos + n_items + 1, ScanOut<1>{{edge_pos}});
        hipLaunchKernelGGL(sg_edges_kernel, dim3(sg_grid(n_items)), block, 0, c->stream, arcs, n_arcs_p, state, edge_pos, edges);
        launches += 3;
    }
    HIP_TRY(c, hipGetLastError());
    PHASE(timer.stop());
    PHASE(read_ctl(c, ctl, h_ctl, kSgCtlWords));
    if (n_items > 0) PHASE(queue_copies(c, {{&n_arcs, n_arcs_p, 8}, {&n_listed, edge_pos + n_items, 8}}));
    HIP_TRY(c, hipStreamSynchronize(c->stream));              // (the second wait: the control words, the arcs and the edges)
    PHASE(timer.seconds(&seconds[1]));
    if (a.kernel_seconds) *a.kernel_seconds = seconds[0] + seconds[1];
    if (a.launches) *a.launches = launches;
    const unsigned long long *e = h_ctl + kSgCtlEnds;
    const long long want_listed = (long long)(a.emit_removed ? h_ctl[kSgCtlEdges] : h_ctl[kSgCtlKeptEdges]);
    if (n_arcs < 0 || n_arcs > n_items || n_listed != want_listed || (long long)h_ctl[kSgCtlViews] != n_items) {
        c->last_error = "string_graph: the scans and the counts disagree";
        return RAFT_HIP_ERR_DEVICE;
    }
    if (a.n_out) *a.n_out = n_listed;
    if (a.sum)
        *a.sum = raft_hip_sg_summary{n_rec, n_items, (int64_t)h_ctl[kSgCtlLeftOut], n_arcs, n_items - n_arcs, (int64_t)h_ctl[kSgCtlUnpaired],
                                     (int64_t)h_ctl[kSgCtlReducible], (int64_t)h_ctl[kSgCtlEdges], (int64_t)(h_ctl[kSgCtlEdges] - h_ctl[kSgCtlKeptEdges]),
                                     (int64_t)h_ctl[kSgCtlKeptEdges], (int64_t)e[0], (int64_t)e[1], (int64_t)e[2], (int64_t)e[3], (int64_t)e[4],
                                     (int64_t)e[5], (int64_t)h_ctl[kSgCtlLongest]};
    const bool wants_edges = a.edge_u || a.edge_w || a.edge_span || a.edge_ext || a.edge_back || a.edge_flags;      // (none: the size query)
    if (wants_edges && n_listed > a.out_cap) return refuse(c, RAFT_HIP_ERR_TOO_LARGE, kWho, "out_cap is below n_out");
    const size_t nn = (size_t)a.n_reads, ne = (size_t)n_listed;
    PHASE(queue_copies(c, {{a.arcs, B[kNodeArcs].p, nn * 8}, {a.kept, B[kNodeKept].p, nn * 8}, {a.partner, B[kPartner].p, nn * 8},
                           {a.span, B[kSpan].p, nn * 8}, {a.flags, B[kFlags].p, nn}, {a.edge_u, edges.u, ne * 4}, {a.edge_w, edges.w, ne * 4},
                           {a.edge_span, edges.span, ne * 4}, {a.edge_ext, edges.ext, ne * 4}, {a.edge_back, edges.back, ne * 4},
                           {a.edge_flags, edges.flags, ne}}));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return RAFT_HIP_OK;
}

} // namespace

extern "C" {

int raft_hip_sg_abi(void) { return RAFT_HIP_ABI_VERSION; }

int raft_hip_string_graph_device(raft_hip_ctx *c, int32_t n_reads, const int32_t *d_read_len, int64_t n_rec, const int32_t *d_qid,
                                 const int32_t *d_qs, const int32_t *d_qe, const int32_t *d_tid, const int32_t *d_ts, const int32_t *d_te,
                                 const uint8_t *d_strand, const uint8_t *d_skip, int32_t max_overhang, int32_t min_ratio_permille,
                                 int32_t symmetric, int32_t fuzz, int32_t emit_removed, int64_t out_cap, int32_t *arcs, int32_t *kept,
                                 int32_t *partner, int32_t *span, uint8_t *flags, int32_t *edge_u, int32_t *edge_w, int32_t *edge_span,
                                 int32_t *edge_ext, int32_t *edge_back, uint8_t *edge_flags, int64_t *n_out, raft_hip_sg_summary *sum,
                                 int64_t *error_index, double *kernel_seconds, int64_t *launches)
{
    const SgCall a{n_reads, d_read_len, {n_rec, {d_qid, d_qs, d_qe, d_tid, d_ts, d_te}}, d_strand, d_skip, max_overhang, min_ratio_permille, symmetric,
                   fuzz, emit_removed, out_cap, arcs, kept, partner, span, flags, edge_u, edge_w, edge_span, edge_ext, edge_back, edge_flags, n_out,
                   sum, error_index, kernel_seconds, launches};
    PHASE(check_call(c, a));
    HIP_TRY(c, hipSetDevice(c->device));
    return sg_run(c, a);
}

// The same from host arrays: the lengths and the six columns staged through q_len and q_col, which no pass uses, the strand bytes and,
// where given, the skip bytes through one staging buffer of this library's own (strand first, skip behind it on a 16-byte line).
int raft_hip_string_graph_host(raft_hip_ctx *c, int32_t n_reads, const int32_t *read_len, int64_t n_rec, const int32_t *qid,
                               const int32_t *qs, const int32_t *qe, const int32_t *tid, const int32_t *ts, const int32_t *te,
                               const uint8_t *strand, const uint8_t *skip, int32_t max_overhang, int32_t min_ratio_permille,
                               int32_t symmetric, int32_t fuzz, int32_t emit_removed, int64_t out_cap, int32_t *arcs, int32_t *kept,
                               int32_t *partner, int32_t *span, uint8_t *flags, int32_t *edge_u, int32_t *edge_w, int32_t *edge_span,
                               int32_t *edge_ext, int32_t *edge_back, uint8_t *edge_flags, int64_t *n_out, raft_hip_sg_summary *sum,
                               int64_t *error_index, double *kernel_seconds, int64_t *launches)
{
    SgCall a{n_reads, read_len, {n_rec, {qid, qs, qe, tid, ts, te}}, strand, skip, max_overhang, min_ratio_permille, symmetric,
             fuzz, emit_removed, out_cap, arcs, kept, partner, span, flags, edge_u, edge_w, edge_span, edge_ext, edge_back, edge_flags, n_out,
             sum, error_index, kernel_seconds, launches};
    PHASE(check_call(c, a));
    HIP_TRY(c, hipSetDevice(c->device));
    PHASE(stage_host(c, c->q_len, read_len, (size_t)n_reads, &a.len));
    const size_t strand_bytes = n_rec > 0 ? ((size_t)n_rec + 15) & ~size_t(15) : 0, skip_bytes = skip && n_reads > 0 ? (size_t)n_reads : 0;
    DevBuf &stage = c->sg[kStage];
    HIP_TRY(c, stage.ensure(std::max<size_t>(strand_bytes + skip_bytes, 1)));
    if (n_rec > 0) {
        PHASE(stage_columns(c, c->q_col, a.rec));
        HIP_TRY(c, hipMemcpyAsync(stage.p, strand, (size_t)n_rec, hipMemcpyHostToDevice, c->stream));
        a.strand = stage.as<uint8_t>();
    }
    if (skip_bytes) {
        HIP_TRY(c, hipMemcpyAsync(stage.as<uint8_t>() + strand_bytes, skip, skip_bytes, hipMemcpyHostToDevice, c->stream));
        a.skip = stage.as<uint8_t>() + strand_bytes;
    }
    return sg_run(c, a);
}

} // extern "C"
