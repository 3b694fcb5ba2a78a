// graph_clean.hpp -- a string graph cleaned on the device (raft_hip_graph_clean_device / _host, include/raft_hip_cln.h): the arc table
// of an edge list, the weak cut, and the tip rounds over the chains that unitig.hpp's list ranking finds.
//
// Kernels, none of which waits for another workgroup (one launch each; graph_clean_lib.hip is the driver):
//   1. cln_items_kernel: a lane per edge runs cln_edge_ok (atomicMin of the first bad edge) and writes the edge's two arcs as items
//      (from, to, item index = 2 * edge + direction); a bad edge's items carry the key 2 * n_reads, which sorts behind every node, so
//      that nothing ever indexes by a value the list gave without a check.  Two stable passes of radix_sort_by_key (sort_pairs.hpp)
//      by `to`, then -- cln_rekey_kernel -- by `from`.  cln_arcs_kernel: a lane per sorted item writes the arc's three columns, the
//      item's place, and compares with the item before it: equal (from, to) is the same unordered pair at a greater index (the sort
//      is stable and an edge's items are 2 e and 2 e + 1), a duplicate.  cln_rows_kernel: row starts [2 n + 1] by binary search.
//   2. cln_node_max_kernel: a lane per node, m(u) and the row's length.  cln_weak_kernel: a lane per edge compares the span with m
//      of both of its nodes and writes the edge's state byte and the live byte of its two arcs (it is the only writer of both).
//   3. Per round: cln_deg_kernel (a lane per node: live degree, the sole live arc), cln_table_kernel (a lane per read: the unitig
//      table of the live graph, "joined" being its MUTUAL bit), utg_rank (unitig.hpp: the init kernel and ceil(log2 2n) rounds of
//      pointer jumping), cln_chain_kernel (a lane per read: its chain's record from the states of its two half-edges),
//      cln_judge_kernel (a lane per read; the read that owns a candidate's attached end walks the row of b and, for each w, the row
//      of w, reading the record of each neighbour's chain: the work is the sum over the candidates of the rows they touch),
//      cln_mark_reads_kernel and cln_mark_edges_kernel.  The judge only reads the graph and the marks only write it, so every chain
//      is judged against the graph as the round found it.
//   4. cln_totals_kernel: a lane per read, the totals over the final graph with one atomic per wave and total.
// No kernel keeps a row in LDS: a row is walked by one lane from global memory, whatever its length.
#pragma once
#include "wave.hpp"
#include "graph_clean_rule.hpp"
#include "unitig.hpp"

namespace raft {

constexpr int kClnThreads = 256, kClnMaxBlocks = 2048;          // eight workgroups on each of the 256 CUs, grid-stride beyond
// control words: the first bad edge, then the counts
constexpr int kClnCtlWeakArcs = 1, kClnCtlWeakEdges = 2, kClnCtlTipReads = 3, kClnCtlTipEdges = 4, kClnCtlTipBases = 5, kClnCtlFlagged = 6, kClnCtlLongest = 7;
constexpr int kClnCtlEnds = 8;               // kept_one, kept_more, mutual, dead, isolated_short
constexpr int kClnEndTotals = 5;
constexpr int kClnCtlUtg = 13;               // the two words utg_init_kernel and utg_jump_kernel take: the first bad read, the half-edges on cycles
constexpr int kClnCtlRoundTips = 16;         // [round]: the chains that fell in it
constexpr int kClnCtlRoundKept = kClnCtlRoundTips + kClnMaxRounds + 1;      // [round]: the candidates that did not
constexpr int kClnCtlWords = kClnCtlRoundKept + kClnMaxRounds + 1;

inline unsigned cln_grid(long long n) { return (unsigned)(n < 1 ? 1 : ((n + kClnThreads - 1) / kClnThreads > kClnMaxBlocks ? kClnMaxBlocks : (n + kClnThreads - 1) / kClnThreads)); }

struct ClnEdgeList { const int32_t *u, *w, *span; long long n; };
// the arcs in (from, to) order
struct ClnArcs { int32_t *to, *edge, *span; uint8_t *live; };

__global__ __launch_bounds__(kClnThreads) void cln_items_kernel(ClnEdgeList ed, int32_t n_reads, const int32_t *__restrict__ len, const uint8_t *__restrict__ skip,
                                                                uint32_t *__restrict__ item_from, uint32_t *__restrict__ key, int32_t *__restrict__ val,
                                                                uint8_t *__restrict__ edge_state, uint8_t *__restrict__ edge_round,
                                                                unsigned long long *__restrict__ ctl)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    const uint32_t nil = 2u * (uint32_t)n_reads;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < ed.n; e += stride) {
        const int32_t u = ed.u[e], w = ed.w[e];
        const bool ok = cln_edge_ok(n_reads, len, skip, u, w, ed.span[e]);
        if (!ok) atomicMin(ctl, (unsigned long long)e);
        item_from[2 * e] = ok ? (uint32_t)u : nil; item_from[2 * e + 1] = ok ? (uint32_t)w : nil;
        key[2 * e] = ok ? (uint32_t)w : nil; key[2 * e + 1] = ok ? (uint32_t)u : nil;
        val[2 * e] = (int32_t)(2 * e); val[2 * e + 1] = (int32_t)(2 * e + 1);
        edge_state[e] = 0; edge_round[e] = 0;
    }
}

__global__ __launch_bounds__(kClnThreads) void cln_rekey_kernel(const int32_t *__restrict__ val, const uint32_t *__restrict__ item_from, long long n_items,
                                                                uint32_t *__restrict__ key)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n_items; p += stride) key[p] = item_from[val[p]];
}

// where item i goes to: the other node of its edge
__device__ __forceinline__ int32_t cln_item_to(const ClnEdgeList &ed, int32_t item) { return (item & 1) ? ed.u[item >> 1] : ed.w[item >> 1]; }

__global__ __launch_bounds__(kClnThreads) void cln_arcs_kernel(const uint32_t *__restrict__ from, const int32_t *__restrict__ val, long long n_items, ClnEdgeList ed,
                                                               int32_t n_reads, ClnArcs arc, int32_t *__restrict__ item_pos, unsigned long long *__restrict__ ctl)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    const uint32_t nil = 2u * (uint32_t)n_reads;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < n_items; p += stride) {
        const int32_t item = val[p];
        const uint32_t f = from[p];
        const int32_t to = cln_item_to(ed, item);
        // (an item with the key nil belongs to a bad edge, which cln_items_kernel has reported: no row holds it)
        if (f != nil && p > 0 && from[p - 1] == f && cln_item_to(ed, val[p - 1]) == to) atomicMin(ctl, (unsigned long long)(item >> 1));
        arc.to[p] = f != nil ? to : -1; arc.edge[p] = item >> 1; arc.span[p] = ed.span[item >> 1]; arc.live[p] = 0;
        item_pos[item] = (int32_t)p;
    }
}

// the first place in a[0, n) (ascending) that holds x or more
__device__ __forceinline__ long long cln_lower_bound(const uint32_t *__restrict__ a, long long n, uint32_t x)
{
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// row[x], x = 0 .. n_nodes: where the arcs of node x begin; row[n_nodes] is where the bad edges' items begin, the end of the last row
__global__ __launch_bounds__(kClnThreads) void cln_rows_kernel(const uint32_t *__restrict__ from, long long n_items, long long n_nodes, int32_t *__restrict__ row)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x; x <= n_nodes; x += stride) row[x] = (int32_t)cln_lower_bound(from, n_items, (uint32_t)x);
}

__device__ __forceinline__ unsigned cln_wave_max(unsigned v)
{
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) {
        const unsigned o = __shfl_xor(v, d, kWave);
        v = o > v ? o : v;
    }
    return v;
}

// per node: m(u), the greatest span of its row (0 for an empty one), and the row's length
__global__ __launch_bounds__(kClnThreads) void cln_node_max_kernel(const int32_t *__restrict__ row, const int32_t *__restrict__ arc_span, long long n_nodes,
                                                                   int32_t *__restrict__ node_max, int32_t *__restrict__ node_arcs,
                                                                   unsigned long long *__restrict__ ctl)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    const int lane = (int)threadIdx.x & (kWave - 1);
    unsigned longest = 0;
    for (long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x; x < n_nodes; x += stride) {
        const int32_t lo = row[x], hi = row[x + 1];
        int32_t m = 0;
        for (int32_t a = lo; a < hi; ++a) m = arc_span[a] > m ? arc_span[a] : m;
        node_max[x] = m; node_arcs[x] = hi - lo;
        longest = (unsigned)(hi - lo) > longest ? (unsigned)(hi - lo) : longest;
    }
    const unsigned m = cln_wave_max(longest);              // (all lanes are back together here)
    if (lane == 0 && m) atomicMax(&ctl[kClnCtlLongest], (unsigned long long)m);
}

// per edge: the weak bits of its two arcs, and whether it lives
__global__ __launch_bounds__(kClnThreads) void cln_weak_kernel(ClnEdgeList ed, int32_t w_permille, const int32_t *__restrict__ node_max,
                                                               const int32_t *__restrict__ item_pos, uint8_t *__restrict__ edge_state,
                                                               uint8_t *__restrict__ arc_live, unsigned long long *__restrict__ ctl)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    const int lane = (int)threadIdx.x & (kWave - 1);
    unsigned tot[2] = {0, 0};                              // weak arcs, weak edges
    for (long long e0 = (long long)blockIdx.x * blockDim.x + ((int)threadIdx.x & ~(kWave - 1)); e0 < ed.n; e0 += stride) {
        const long long e = e0 + lane;
        if (e < ed.n) {
            const int32_t span = ed.span[e];
            const bool wu = cln_weak(span, w_permille, node_max[ed.u[e]]), ww = cln_weak(span, w_permille, node_max[ed.w[e]]);
            const unsigned st = (wu ? (unsigned)kClnWeakU : 0u) | (ww ? (unsigned)kClnWeakW : 0u);
            edge_state[e] = (uint8_t)st;
            arc_live[item_pos[2 * e]] = st ? 0 : 1; arc_live[item_pos[2 * e + 1]] = st ? 0 : 1;
            tot[0] += (wu ? 1u : 0u) + (ww ? 1u : 0u); tot[1] += st ? 1u : 0u;
        }
    }
    wave_flush_totals(tot, &ctl[kClnCtlWeakArcs], lane);   // (all lanes are back together here)
}

// per read: its state before the rounds
__global__ __launch_bounds__(kClnThreads) void cln_reads_kernel(int32_t n_reads, const uint8_t *__restrict__ skip, uint8_t *__restrict__ read_state,
                                                                uint8_t *__restrict__ read_round, uint8_t *__restrict__ verdict, unsigned long long *__restrict__ ctl)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    const int lane = (int)threadIdx.x & (kWave - 1);
    unsigned tot[1] = {0};
    for (long long r0 = (long long)blockIdx.x * blockDim.x + ((int)threadIdx.x & ~(kWave - 1)); r0 < n_reads; r0 += stride) {
        const long long r = r0 + lane;
        if (r < n_reads) {
            const bool flagged = skip && skip[r];
            read_state[r] = (uint8_t)(flagged ? kClnReadFlagged : kClnReadStays); read_round[r] = 0; verdict[r] = 0;
            tot[0] += flagged ? 1u : 0u;
        }
    }
    wave_flush_totals(tot, &ctl[kClnCtlFlagged], lane);    // (all lanes are back together here)
}

// per node: the live arcs of its row and, where there is one, that arc (-1 otherwise); with `weak`, what the row has lost
__global__ __launch_bounds__(kClnThreads) void cln_deg_kernel(const int32_t *__restrict__ row, const uint8_t *__restrict__ arc_live, long long n_nodes,
                                                              int32_t *__restrict__ deg, int32_t *__restrict__ sole, int32_t *__restrict__ weak)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x; x < n_nodes; x += stride) {
        const int32_t lo = row[x], hi = row[x + 1];
        int32_t k = 0, last = -1;
        for (int32_t a = lo; a < hi; ++a)
            if (arc_live[a]) { k += 1; last = a; }
        deg[x] = k; sole[x] = k == 1 ? last : -1;
        if (weak) weak[x] = hi - lo - k;
    }
}

// per read: the unitig table of the live graph -- an end is MUTUAL where it is joined
__global__ __launch_bounds__(kClnThreads) void cln_table_kernel(int32_t n_reads, const uint8_t *__restrict__ read_state, const int32_t *__restrict__ arc_to,
                                                                const int32_t *__restrict__ arc_span, const int32_t *__restrict__ deg,
                                                                const int32_t *__restrict__ sole, int32_t *__restrict__ partner, int32_t *__restrict__ span,
                                                                uint8_t *__restrict__ flags)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += stride) {
        unsigned flag = read_state[r] != kClnReadStays ? (unsigned)kBestSkipped : 0u;
        int p[2] = {-1, -1}, s[2] = {0, 0};
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int32_t u = (int32_t)(2 * r + e);
            if (deg[u] != 1) continue;
            const int32_t a = sole[u], w = arc_to[a];
            if (deg[w] != 1) continue;                     // (the sole live arc of w is then the twin: both arcs of an edge live together)
            p[e] = w >> 1; s[e] = arc_span[a];
            flag |= (((w & 1) == e ? (unsigned)kBestRev5 : 0u) | (unsigned)kBestMutual5) << (2 * e);
        }
        *reinterpret_cast<int2 *>(partner + 2 * r) = make_int2(p[0], p[1]);
        *reinterpret_cast<int2 *>(span + 2 * r) = make_int2(s[0], s[1]);
        flags[r] = (uint8_t)flag;
    }
}

// per read: the record of its chain, from the walks that leave its two ends
__global__ __launch_bounds__(kClnThreads) void cln_chain_kernel(const UtgState *__restrict__ state, int32_t n_reads, const int32_t *__restrict__ len,
                                                                const uint8_t *__restrict__ read_state, const int32_t *__restrict__ deg, int32_t max_tip_reads,
                                                                ClnChain *__restrict__ chain)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += stride) {
        ClnChain c{0, (int32_t)r, 0, {-1, -1}, -1, 0};
        if (read_state[r] == kClnReadStays) {
            const UtgState s0 = state[2 * r], s1 = state[2 * r + 1];
            // a walk still under way after the ranking's rounds goes round a cycle
            c.circular = (s0.next >= 0 || s1.next >= 0) ? 1 : 0;
            c.reads = 1 + s0.cnt + s1.cnt;
            c.length = (int64_t)utg_len(len[r]) + s0.w + s1.w;
            c.first = s0.min < s1.min ? s0.min : s1.min;
            c.term[0] = s0.last; c.term[1] = s1.last;
            if (!c.circular) {
                const int32_t d0 = deg[s0.last], d1 = deg[s1.last];
                if (cln_candidate(false, d0, d1, c.reads, max_tip_reads)) c.attached = d0 == 0 ? s1.last : s0.last;
            }
        }
        chain[r] = c;
    }
}

// per candidate, at the read of its attached end: does it fall?  verdict[that read] = round if it does.
__global__ __launch_bounds__(kClnThreads) void cln_judge_kernel(int32_t n_reads, const ClnChain *__restrict__ chain, const int32_t *__restrict__ row,
                                                                const int32_t *__restrict__ arc_to, const uint8_t *__restrict__ arc_live, int32_t round,
                                                                uint8_t *__restrict__ verdict, unsigned long long *__restrict__ ctl)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    const int lane = (int)threadIdx.x & (kWave - 1);
    unsigned tot[1] = {0};                                 // chains that fell
    unsigned kept = 0;
    long long bases = 0;
    for (long long r0 = (long long)blockIdx.x * blockDim.x + ((int)threadIdx.x & ~(kWave - 1)); r0 < n_reads; r0 += stride) {
        const long long r = r0 + lane;
        if (r < n_reads) {
            const ClnChain c = chain[r];
            if (c.attached >= 0 && (c.attached >> 1) == (int32_t)r) {
                const int32_t b = c.attached;
                bool falls = true;
                for (int32_t a = row[b]; a < row[b + 1] && falls; ++a) {
                    if (!arc_live[a]) continue;
                    const int32_t w = arc_to[a];
                    bool beaten = false;
                    for (int32_t t = row[w]; t < row[w + 1] && !beaten; ++t) {
                        if (!arc_live[t]) continue;
                        const int32_t x = arc_to[t];
                        if (x != b && cln_beats(chain[x >> 1], c)) beaten = true;
                    }
                    falls = beaten;
                }
                if (falls) { verdict[r] = (uint8_t)round; tot[0] += 1; bases += c.length; }
                else kept += 1;
            }
        }
    }
    // (all lanes are back together here)
    wave_flush_totals(tot, &ctl[kClnCtlRoundTips + round], lane);
    const unsigned k = (unsigned)wave_reduce_add((int)kept);
    const long long tb = wave_reduce_add64(bases);
    if (lane == 0 && k) atomicAdd(&ctl[kClnCtlRoundKept + round], (unsigned long long)k);
    if (lane == 1 && tb) atomicAdd(&ctl[kClnCtlTipBases], (unsigned long long)tb);
}

// per read: removed with its chain
__global__ __launch_bounds__(kClnThreads) void cln_mark_reads_kernel(int32_t n_reads, const ClnChain *__restrict__ chain, const uint8_t *__restrict__ verdict,
                                                                     int32_t round, uint8_t *__restrict__ read_state, uint8_t *__restrict__ read_round,
                                                                     unsigned long long *__restrict__ ctl)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    const int lane = (int)threadIdx.x & (kWave - 1);
    unsigned tot[1] = {0};
    for (long long r0 = (long long)blockIdx.x * blockDim.x + ((int)threadIdx.x & ~(kWave - 1)); r0 < n_reads; r0 += stride) {
        const long long r = r0 + lane;
        if (r < n_reads) {
            const int32_t b = chain[r].attached;
            if (b >= 0 && verdict[b >> 1] == (uint8_t)round) { read_state[r] = (uint8_t)kClnReadTip; read_round[r] = (uint8_t)round; tot[0] += 1; }
        }
    }
    wave_flush_totals(tot, &ctl[kClnCtlTipReads], lane);   // (all lanes are back together here)
}

// per edge: a live edge that touches a removed read falls with it
__global__ __launch_bounds__(kClnThreads) void cln_mark_edges_kernel(ClnEdgeList ed, const uint8_t *__restrict__ read_state, const int32_t *__restrict__ item_pos,
                                                                     int32_t round, uint8_t *__restrict__ edge_state, uint8_t *__restrict__ edge_round,
                                                                     uint8_t *__restrict__ arc_live, unsigned long long *__restrict__ ctl)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    const int lane = (int)threadIdx.x & (kWave - 1);
    unsigned tot[1] = {0};
    for (long long e0 = (long long)blockIdx.x * blockDim.x + ((int)threadIdx.x & ~(kWave - 1)); e0 < ed.n; e0 += stride) {
        const long long e = e0 + lane;
        if (e < ed.n && edge_state[e] == 0 && (read_state[ed.u[e] >> 1] == kClnReadTip || read_state[ed.w[e] >> 1] == kClnReadTip)) {
            edge_state[e] = (uint8_t)kClnTip; edge_round[e] = (uint8_t)round;
            arc_live[item_pos[2 * e]] = 0; arc_live[item_pos[2 * e + 1]] = 0;
            tot[0] += 1;
        }
    }
    wave_flush_totals(tot, &ctl[kClnCtlTipEdges], lane);   // (all lanes are back together here)
}

// per read: the totals over the final graph's ends and chains
__global__ __launch_bounds__(kClnThreads) void cln_totals_kernel(int32_t n_reads, const uint8_t *__restrict__ read_state, const uint8_t *__restrict__ flags,
                                                                 const int32_t *__restrict__ deg, const ClnChain *__restrict__ chain, int32_t max_tip_reads,
                                                                 unsigned long long *__restrict__ ctl)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    const int lane = (int)threadIdx.x & (kWave - 1);
    unsigned tot[kClnEndTotals] = {};                      // kept_one, kept_more, mutual, dead, isolated_short
    for (long long r0 = (long long)blockIdx.x * blockDim.x + ((int)threadIdx.x & ~(kWave - 1)); r0 < n_reads; r0 += stride) {
        const long long r = r0 + lane;
        if (r < n_reads) {
            const bool stays = read_state[r] == kClnReadStays;
            const unsigned f = flags[r];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int32_t k = deg[2 * r + e];
                tot[0] += k == 1 ? 1u : 0u; tot[1] += k >= 2 ? 1u : 0u; tot[2] += utg_mutual(f, e) ? 1u : 0u; tot[3] += (stays && k == 0) ? 1u : 0u;
            }
            const ClnChain c = chain[r];
            if (stays && c.first == (int32_t)r && cln_isolated_short(c.circular != 0, deg[c.term[0]], deg[c.term[1]], c.reads, max_tip_reads)) tot[4] += 1;
        }
    }
    wave_flush_totals(tot, &ctl[kClnCtlEnds], lane);       // (all lanes are back together here)
}

} // namespace raft
