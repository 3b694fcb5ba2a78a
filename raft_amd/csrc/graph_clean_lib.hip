// graph_clean_lib.hip -- libraft_hip_cln.so: raft_hip_graph_clean_device / _host (include/raft_hip_cln.h), a string graph cleaned: the
// edges that are weak beside the best one at the same read end cut, the short dead-end chains removed over several rounds.
//
// A library of its own beside libraft_hip.so (the others: the SIDE list of raft_amd/csrc/Makefile): the set of entry points of
// include/raft_hip.h is closed (ABI 11), and this call needs nothing of the engine but the context it is handed -- the stream, and
// buffers registered with the context like every other (cln[], and the queries' shared staging q_len, q_col).  It reads no finished
// pass and leaves the context's state as it is.
//
// The call waits once behind the arc table, where the first bad edge is read, once per round for the number of chains that fell,
// and once behind the last launch, where the control words are read: R + 2 waits at most.
#include "query_host.hpp"
#include "../../include/raft_hip_cln.h"
#include "sort_pairs.hpp"
#include "graph_clean.hpp"

namespace {

// the context's cln[] by name
enum ClnBuf {
    kItemFrom, kKeyA, kKeyB, kValA, kValB, kSortTmp, kArcTo, kArcEdge, kArcSpan, kArcLive, kItemPos, kRow, kNodeMax, kNodeArcs, kNodeWeak, kDeg, kSole,
    kEdgeState, kEdgeRound, kReadState, kReadRound, kVerdict, kPartner, kSpan, kFlags, kState, kChain, kCtl, kStage, kClnBufCount
};
static_assert(kClnBufCount == kClnBufs, "engine_ctx.hpp's count of this library's buffers");

struct ClnCall {
    int32_t n_reads;
    const int32_t *len;
    const uint8_t *skip;
    int64_t n_edges;
    const int32_t *edge_u, *edge_w, *edge_span;
    int32_t min_ratio, max_tip_reads, rounds;
    uint8_t *edge_state, *edge_round, *read_state, *read_round;
    int32_t *arcs, *weak, *kept, *partner, *span; uint8_t *flags;
    raft_hip_cln_summary *sum; int64_t *error_index; double *kernel_seconds; int64_t *launches;
};

constexpr const char *kWho = "graph_clean";
constexpr const char *kBadEdge = "graph_clean: an edge names a node outside [0, 2 * n_reads), one read twice or a flagged read, has a span "
                                 "outside [1, the shorter length], or repeats a pair (error_index: the edge)";
static_assert(RAFT_HIP_CLN_WEAK_U == kClnWeakU && RAFT_HIP_CLN_WEAK_W == kClnWeakW && RAFT_HIP_CLN_TIP == kClnTip, "the edge bits of the header");
static_assert(RAFT_HIP_CLN_READ_STAYS == kClnReadStays && RAFT_HIP_CLN_READ_TIP == kClnReadTip && RAFT_HIP_CLN_READ_FLAGGED == kClnReadFlagged,
              "the read states of the header");

// what both forms check before anything is staged
int check_call(raft_hip_ctx *c, const ClnCall &a)
{
    if (!c) return RAFT_HIP_ERR_PARAM;
    if (a.min_ratio < 0 || a.min_ratio > 1000) return refuse(c, RAFT_HIP_ERR_PARAM, kWho, "min_ratio_permille outside [0, 1000]");
    if (a.max_tip_reads < 0) return refuse(c, RAFT_HIP_ERR_PARAM, kWho, "max_tip_reads is negative");
    if (a.rounds < 1 || a.rounds > kClnMaxRounds) return refuse(c, RAFT_HIP_ERR_PARAM, kWho, "rounds outside [1, 64]");
    if (a.n_reads < 0) return refuse(c, RAFT_HIP_ERR_PARAM, kWho, "n_reads is negative");
    if (a.n_edges < 0) return refuse(c, RAFT_HIP_ERR_PARAM, kWho, "n_edges is negative");
    if (a.n_reads > 0 && !a.len) return refuse(c, RAFT_HIP_ERR_PARAM, kWho, "read_len is missing");
    if (a.n_edges > 0 && (!a.edge_u || !a.edge_w || !a.edge_span)) return refuse(c, RAFT_HIP_ERR_PARAM, kWho, "a missing column (edge_u, edge_w, edge_span)");
    if (a.n_reads > kUtgMaxReads || a.n_edges >= (int64_t(1) << 30))
        return refuse(c, RAFT_HIP_ERR_TOO_LARGE, kWho, "more than 2^30 - 1 reads or 2^30 edges or more: nodes and arcs are int32");
    return RAFT_HIP_OK;
}

int bits_for(long long n_values)
{
    int bits = 1;
    while (bits < 32 && (1ll << bits) < n_values) bits += 1;
    return bits;
}

// one span of launches has been queued: wait for it and add its device time
int wait_span(raft_hip_ctx *c, const ClnCall &a, QueryTimer &timer, double *seconds, int64_t launches)
{
    double part = 0.0;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    PHASE(timer.seconds(&part));
    *seconds += part;
    if (a.kernel_seconds) *a.kernel_seconds = *seconds;
    if (a.launches) *a.launches = launches;
    return RAFT_HIP_OK;
}

// a: device arrays but for the outputs
int cln_run(raft_hip_ctx *c, const ClnCall &a)
{
    if (a.kernel_seconds) *a.kernel_seconds = 0.0;
    if (a.launches) *a.launches = 0;
    if (a.n_reads == 0) {                                  // (no node: every edge is bad, the first one first)
        if (a.n_edges > 0) return first_bad_record(c, 0, a.error_index, kBadEdge);
        if (a.error_index) *a.error_index = -1;
        if (a.sum) { *a.sum = raft_hip_cln_summary{}; a.sum->rounds_run = 1; a.sum->converged = 1; }
        return RAFT_HIP_OK;
    }
    const size_t n = (size_t)a.n_reads, ne = (size_t)a.n_edges, m = std::max<size_t>(2 * ne, 1);
    const long long n_nodes = 2ll * a.n_reads, n_items = 2ll * a.n_edges;
    auto &B = c->cln;
    for (int k : {kItemFrom, kKeyA, kKeyB, kValA, kValB, kArcTo, kArcEdge, kArcSpan, kItemPos}) HIP_TRY(c, B[k].ensure(m * 4));
    HIP_TRY(c, B[kArcLive].ensure(m));
    HIP_TRY(c, B[kSortTmp].ensure(rs_tmp_bytes<int32_t>(n_items)));
    HIP_TRY(c, B[kRow].ensure((2 * n + 1) * 4));
    for (int k : {kNodeMax, kNodeArcs, kNodeWeak, kDeg, kSole, kPartner, kSpan}) HIP_TRY(c, B[k].ensure(2 * n * 4));
    for (int k : {kEdgeState, kEdgeRound}) HIP_TRY(c, B[k].ensure(std::max<size_t>(ne, 1)));
    for (int k : {kReadState, kReadRound, kVerdict, kFlags}) HIP_TRY(c, B[k].ensure(n));
    HIP_TRY(c, B[kState].ensure(n * 4 * sizeof(UtgState)));               // two half-edges per read, two halves
    HIP_TRY(c, B[kChain].ensure(n * sizeof(ClnChain)));
    HIP_TRY(c, B[kCtl].ensure((size_t)kClnCtlWords * 8));
    QueryTimer timer(c, a.kernel_seconds);
    unsigned long long *ctl = B[kCtl].as<unsigned long long>();
    unsigned long long h_ctl[kClnCtlWords] = {};
    int64_t launches = 0;
    double seconds = 0.0;
    const ClnEdgeList ed{a.edge_u, a.edge_w, a.edge_span, (long long)a.n_edges};
    const ClnArcs arc{B[kArcTo].as<int32_t>(), B[kArcEdge].as<int32_t>(), B[kArcSpan].as<int32_t>(), B[kArcLive].as<uint8_t>()};
    int32_t *row = B[kRow].as<int32_t>(), *item_pos = B[kItemPos].as<int32_t>(), *deg = B[kDeg].as<int32_t>(), *sole = B[kSole].as<int32_t>();
    uint8_t *edge_state = B[kEdgeState].as<uint8_t>(), *edge_round = B[kEdgeRound].as<uint8_t>();
    uint8_t *read_state = B[kReadState].as<uint8_t>(), *read_round = B[kReadRound].as<uint8_t>(), *verdict = B[kVerdict].as<uint8_t>();
    int32_t *partner = B[kPartner].as<int32_t>(), *span = B[kSpan].as<int32_t>();
    uint8_t *flags = B[kFlags].as<uint8_t>();
    ClnChain *chain = B[kChain].as<ClnChain>();
    const dim3 block(kClnThreads), egrid(cln_grid(a.n_edges)), igrid(cln_grid(n_items)), ngrid(cln_grid(n_nodes)), rgrid(cln_grid(a.n_reads));

    // 1. the arc table and the list's check
    PHASE(clear_ctl(c, ctl, kClnCtlWords));
    HIP_TRY(c, hipMemsetAsync(ctl + kClnCtlUtg, 0xFF, 8, c->stream));     // (the ranking's first bad read: none)
    PHASE(timer.start());
    if (a.n_edges > 0) {
        uint32_t *key[2] = {B[kKeyA].as<uint32_t>(), B[kKeyB].as<uint32_t>()};
        int32_t *val[2] = {B[kValA].as<int32_t>(), B[kValB].as<int32_t>()};
        uint32_t *item_from = B[kItemFrom].as<uint32_t>();
        hipLaunchKernelGGL(cln_items_kernel, egrid, block, 0, c->stream, ed, a.n_reads, a.len, a.skip, item_from, key[0], val[0], edge_state, edge_round, ctl);
        // by `to`, then (stable) by `from`; the keys run to 2 * n_reads, the key of a bad edge's items
        const int bits = bits_for(n_nodes + 1);
        long long sort_launches = 0;
        bool in_b = false;
        HIP_TRY(c, radix_sort_by_key<int32_t>(c->stream, key[0], val[0], key[1], val[1], n_items, bits, B[kSortTmp].p, &in_b, &sort_launches));
        int at = in_b ? 1 : 0;
        hipLaunchKernelGGL(cln_rekey_kernel, igrid, block, 0, c->stream, val[at], item_from, n_items, key[at]);
        HIP_TRY(c, radix_sort_by_key<int32_t>(c->stream, key[at], val[at], key[1 - at], val[1 - at], n_items, bits, B[kSortTmp].p, &in_b, &sort_launches));
        if (in_b) at = 1 - at;
        hipLaunchKernelGGL(cln_arcs_kernel, igrid, block, 0, c->stream, key[at], val[at], n_items, ed, a.n_reads, arc, item_pos, ctl);
        hipLaunchKernelGGL(cln_rows_kernel, dim3(cln_grid(n_nodes + 1)), block, 0, c->stream, key[at], n_items, n_nodes, row);
        launches += 4 + sort_launches;
    } else {
        HIP_TRY(c, hipMemsetAsync(row, 0, (2 * n + 1) * 4, c->stream));
    }
    HIP_TRY(c, hipGetLastError());
    PHASE(timer.stop());
    PHASE(read_ctl(c, ctl, h_ctl, 1));
    PHASE(wait_span(c, a, timer, &seconds, launches));       // (the first wait: nothing below indexes by an edge that was not checked)
    PHASE(first_bad_record(c, h_ctl[0], a.error_index, kBadEdge));

    // 2. the weak cut, the reads' states
    PHASE(timer.start());
    hipLaunchKernelGGL(cln_node_max_kernel, ngrid, block, 0, c->stream, row, arc.span, n_nodes, B[kNodeMax].as<int32_t>(), B[kNodeArcs].as<int32_t>(), ctl);
    if (a.n_edges > 0) {
        hipLaunchKernelGGL(cln_weak_kernel, egrid, block, 0, c->stream, ed, a.min_ratio, B[kNodeMax].as<int32_t>(), item_pos, edge_state, arc.live, ctl);
        launches += 1;
    }
    hipLaunchKernelGGL(cln_reads_kernel, rgrid, block, 0, c->stream, a.n_reads, a.skip, read_state, read_round, verdict, ctl);
    launches += 2;

    // 3. the rounds; survey(): degrees, the table, the ranking and the chain records of the live graph
    const int rank_rounds = utg_rounds(a.n_reads);
    UtgState *const half[2] = {B[kState].as<UtgState>(), B[kState].as<UtgState>() + n_nodes};
    auto survey = [&](int32_t *weak) {
        hipLaunchKernelGGL(cln_deg_kernel, ngrid, block, 0, c->stream, row, arc.live, n_nodes, deg, sole, weak);
        hipLaunchKernelGGL(cln_table_kernel, rgrid, block, 0, c->stream, a.n_reads, read_state, arc.to, arc.span, deg, sole, partner, span, flags);
        const UtgState *state = utg_rank(c->stream, a.n_reads, a.len, partner, span, flags, nullptr, half, ctl + kClnCtlUtg, rank_rounds, false, &launches);
        hipLaunchKernelGGL(cln_chain_kernel, rgrid, block, 0, c->stream, state, a.n_reads, a.len, read_state, deg, a.max_tip_reads, chain);
        launches += 3;
    };
    int rounds_run = 0, converged = 0;
    long long tips = 0;
    for (int k = 1; k <= a.rounds && !converged; ++k) {
        if (k > 1) PHASE(timer.start());
        survey(k == 1 ? B[kNodeWeak].as<int32_t>() : nullptr);
        hipLaunchKernelGGL(cln_judge_kernel, rgrid, block, 0, c->stream, a.n_reads, chain, row, arc.to, arc.live, k, verdict, ctl);
        hipLaunchKernelGGL(cln_mark_reads_kernel, rgrid, block, 0, c->stream, a.n_reads, chain, verdict, k, read_state, read_round, ctl);
        launches += 2;
        if (a.n_edges > 0) {
            hipLaunchKernelGGL(cln_mark_edges_kernel, egrid, block, 0, c->stream, ed, read_state, item_pos, k, edge_state, edge_round, arc.live, ctl);
            launches += 1;
        }
        HIP_TRY(c, hipGetLastError());
        PHASE(timer.stop());
        PHASE(read_ctl(c, ctl + kClnCtlRoundTips + k, h_ctl + kClnCtlRoundTips + k, 1));
        PHASE(wait_span(c, a, timer, &seconds, launches));   // (a round's wait: did anything fall?)
        rounds_run = k;
        tips += (long long)h_ctl[kClnCtlRoundTips + k];
        converged = h_ctl[kClnCtlRoundTips + k] == 0 ? 1 : 0;
    }

    // 4. the final graph: the last round's survey holds it if nothing fell there
    PHASE(timer.start());
    if (!converged) survey(nullptr);
    hipLaunchKernelGGL(cln_totals_kernel, rgrid, block, 0, c->stream, a.n_reads, read_state, flags, deg, chain, a.max_tip_reads, ctl);
    launches += 1;
    HIP_TRY(c, hipGetLastError());
    PHASE(timer.stop());
    PHASE(read_ctl(c, ctl, h_ctl, kClnCtlWords));
    PHASE(queue_copies(c, {{a.edge_state, edge_state, ne}, {a.edge_round, edge_round, ne}, {a.read_state, read_state, n}, {a.read_round, read_round, n},
                           {a.arcs, B[kNodeArcs].p, n * 8}, {a.weak, B[kNodeWeak].p, n * 8}, {a.kept, deg, n * 8}, {a.partner, partner, n * 8},
                           {a.span, span, n * 8}, {a.flags, flags, n}}));
    PHASE(wait_span(c, a, timer, &seconds, launches));       // (the last wait: the control words and the copies)
    if (h_ctl[kClnCtlUtg] != ~0ull) {
        c->last_error = "graph_clean: the table of the live graph is inconsistent";
        return RAFT_HIP_ERR_DEVICE;
    }
    const unsigned long long *e = h_ctl + kClnCtlEnds;
    if (a.sum)
        *a.sum = raft_hip_cln_summary{(int64_t)a.n_reads, (int64_t)h_ctl[kClnCtlFlagged], a.n_edges, (int64_t)h_ctl[kClnCtlWeakArcs],
                                      (int64_t)h_ctl[kClnCtlWeakEdges], rounds_run, converged, tips, (int64_t)h_ctl[kClnCtlTipReads],
                                      (int64_t)h_ctl[kClnCtlTipBases], (int64_t)h_ctl[kClnCtlTipEdges], (int64_t)h_ctl[kClnCtlRoundKept + rounds_run],
                                      (int64_t)e[4], a.n_edges - (int64_t)h_ctl[kClnCtlWeakEdges] - (int64_t)h_ctl[kClnCtlTipEdges], (int64_t)e[0],
                                      (int64_t)e[1], (int64_t)e[2], (int64_t)e[3], (int64_t)h_ctl[kClnCtlLongest]};
    return RAFT_HIP_OK;
}

} // namespace

extern "C" {

int raft_hip_cln_abi(void) { return RAFT_HIP_ABI_VERSION; }

int raft_hip_graph_clean_device(raft_hip_ctx *c, int32_t n_reads, const int32_t *d_read_len, const uint8_t *d_skip, int64_t n_edges,
                                const int32_t *d_edge_u, const int32_t *d_edge_w, const int32_t *d_edge_span, int32_t min_ratio_permille,
                                int32_t max_tip_reads, int32_t rounds, uint8_t *edge_state, uint8_t *edge_round, uint8_t *read_state,
                                uint8_t *read_round, int32_t *arcs, int32_t *weak, int32_t *kept, int32_t *partner, int32_t *span,
                                uint8_t *flags, raft_hip_cln_summary *sum, int64_t *error_index, double *kernel_seconds, int64_t *launches)
{
    const ClnCall a{n_reads, d_read_len, d_skip, n_edges, d_edge_u, d_edge_w, d_edge_span, min_ratio_permille, max_tip_reads, rounds, edge_state,
                    edge_round, read_state, read_round, arcs, weak, kept, partner, span, flags, sum, error_index, kernel_seconds, launches};
    PHASE(check_call(c, a));
    HIP_TRY(c, hipSetDevice(c->device));
    return cln_run(c, a);
}

// The same from host arrays: the lengths staged through q_len, the three edge columns through q_col[0 .. 2], which no pass uses, the
// skip bytes, where given, through a staging buffer of this library's own.
int raft_hip_graph_clean_host(raft_hip_ctx *c, int32_t n_reads, const int32_t *read_len, const uint8_t *skip, int64_t n_edges,
                              const int32_t *edge_u, const int32_t *edge_w, const int32_t *edge_span, int32_t min_ratio_permille,
                              int32_t max_tip_reads, int32_t rounds, uint8_t *edge_state, uint8_t *edge_round, uint8_t *read_state,
                              uint8_t *read_round, int32_t *arcs, int32_t *weak, int32_t *kept, int32_t *partner, int32_t *span,
                              uint8_t *flags, raft_hip_cln_summary *sum, int64_t *error_index, double *kernel_seconds, int64_t *launches)
{
    ClnCall a{n_reads, read_len, skip, n_edges, edge_u, edge_w, edge_span, min_ratio_permille, max_tip_reads, rounds, edge_state,
              edge_round, read_state, read_round, arcs, weak, kept, partner, span, flags, sum, error_index, kernel_seconds, launches};
    PHASE(check_call(c, a));
    HIP_TRY(c, hipSetDevice(c->device));
    if (n_reads > 0) {
        PHASE(stage_host(c, c->q_len, read_len, (size_t)n_reads, &a.len));
        if (skip) PHASE(stage_host(c, c->cln[kStage], skip, (size_t)n_reads, &a.skip));
    }
    if (n_edges > 0 && n_reads > 0) {
        PHASE(stage_host(c, c->q_col[0], edge_u, (size_t)n_edges, &a.edge_u));
        PHASE(stage_host(c, c->q_col[1], edge_w, (size_t)n_edges, &a.edge_w));
        PHASE(stage_host(c, c->q_col[2], edge_span, (size_t)n_edges, &a.edge_span));
    }
    return cln_run(c, a);
}

} // extern "C"
