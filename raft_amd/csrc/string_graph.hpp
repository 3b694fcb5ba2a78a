// string_graph.hpp -- the string graph of a record stream (raft_hip_string_graph_device / _host, include/raft_hip_sg.h): the arcs of the
// dovetail views compacted out of the stream, sorted by (u, w), one chosen per (u, w), the reducible ones flagged row by row, the
// flags made symmetric, and the tables and the edge list written from that.
//
// Kernels, none of which waits for another workgroup (one launch each):
//   1. best_digest_kernel (best_ovl.hpp): len | skipped << 31 per read.
//      sg_count_kernel: one streaming pass of record_stream.hpp's shape -- the six columns and the lane's four strand bytes (25 B per
//      record in), the two digests gathered, ends_kind.  Per lane group (four records) one byte goes out: bit 2 i the query view of
//      record i gives an arc, bit 2 i + 1 its target view does; per wave step (256 records) the number of set bits.  One exclusive
//      scan (device_scan.hpp) over the steps' counts -- 1 / 256 of the records -- and sg_fill_kernel, which reads the bytes, places
//      its lanes by a wave scan behind the step's offset and loads the records only where a byte is not 0: on a stream that is
//      sparse in dovetails the second pass reads a quarter of a byte per record and little else.  Nothing behind this is sized by
//      the records in traffic, only by the views that give an arc (the items).
//   2. Two stable passes of radix_sort_by_key (sort_pairs.hpp) over (key, item index): by w, then -- sg_rekey_kernel writes u over
//      the keys in the order the first pass left -- by u, each over the bits that 2 * n_reads needs.
//   3. sg_choose_kernel: a lane per sorted item; the first item of a run of one (u, w) is its head, and the head walks its run and
//      keeps the item with the greatest key -- a segmented maximum whose segments are a handful of items (several records of one
//      pair of read ends).  One scan over the head flags, sg_compact_kernel (the chosen arcs as five columns in (u, w) order), and
//      sg_rows_kernel: where every node's row begins, [2 * n_reads + 1], by binary search in the sorted u column.
//   4. sg_reduce_kernel: a wave per row.  A wave takes 64 consecutive nodes, finds the rows of two arcs or more with one ballot and
//      takes them in turn: w and ext of the row into LDS up to kSgRowLds arcs (read from global memory beyond that), then the lanes
//      run over the (arc, via) pairs of the row, 64 at a time; the target is looked up in the row of via ^ 1 by binary search (a
//      row is sorted by w).  One flag byte per arc; lanes that flag the same arc store the same byte.  The work is the row length
//      squared, by the nature of the rule.
//   5. sg_pair_kernel: a lane per arc looks its twin up by binary search and writes the arc's state byte (reducible here, reducible
//      there, unpaired, survives, is listed).  sg_ends_kernel: a lane per node counts the survivors of its row and keeps the one
//      where there is one.  sg_table_kernel: a lane per read writes the unitig table and the totals.  One scan over "is listed"
//      and sg_edges_kernel, which writes the list.
#pragma once
#include "record_stream.hpp"
#include "ovl_ends_rule.hpp"
#include "string_graph_rule.hpp"
#include "best_ovl.hpp"

#ifndef RAFT_SG_ROW_LDS
#define RAFT_SG_ROW_LDS 256                  // arcs of a row the reduction keeps in LDS (w and ext: 8 bytes each)
#endif

namespace raft {

constexpr int kSgRowLds = RAFT_SG_ROW_LDS;
constexpr int kSgThreads = 256, kSgMaxBlocks = 2048;
// control words: the first bad record, then the counts
constexpr int kSgCtlViews = 1, kSgCtlLeftOut = 2, kSgCtlUnpaired = 3, kSgCtlReducible = 4, kSgCtlEdges = 5, kSgCtlKeptEdges = 6;
constexpr int kSgCtlEnds = 7;                // ends_with_arc, kept_one, kept_more, mutual, dead, reads_flagged
constexpr int kSgEndTotals = 6, kSgCtlLongest = kSgCtlEnds + kSgEndTotals, kSgCtlWords = kSgCtlLongest + 1;
// an arc's state byte
constexpr unsigned kSgStRed = 1, kSgStTwinRed = 2, kSgStUnpaired = 4, kSgStSurvives = 8, kSgStListed = 16;

inline unsigned sg_grid(long long n) { return (unsigned)(n < 1 ? 1 : ((n + kSgThreads - 1) / kSgThreads > kSgMaxBlocks ? kSgMaxBlocks : (n + kSgThreads - 1) / kSgThreads)); }
inline long long sg_groups(long long n_rec) { return (n_rec + kStreamLaneRecords - 1) / kStreamLaneRecords; }
inline long long sg_steps(long long n_rec) { return (sg_groups(n_rec) + kWave - 1) / kWave; }

struct SgStreamArgs {
    const unsigned *dig;                     // [n_reads]: len | skipped << 31
    const int32_t *qid, *qs, *qe, *tid, *ts, *te;
    const uint8_t *strand;
    long long n_rec;
    int32_t n_reads, max_overhang, min_ratio, symmetric;
    uint8_t *mask;                           // [groups]
    int32_t *step_cnt;                       // [steps]
    unsigned long long *ctl;
};

template <bool kVec>
__global__ __launch_bounds__(kStreamThreads) void sg_count_kernel(SgStreamArgs A)
{
    constexpr int R = kStreamLaneRecords;
    const int lane = (int)threadIdx.x & (kWave - 1);
    const unsigned n_reads = (unsigned)A.n_reads;
    const unsigned views = A.symmetric ? 1u : 2u;
    unsigned tot[2] = {0, 0};                              // views that give an arc, views left out
    stream_for_each_group(A.n_rec, lane, [&](const long long first) {
        LaneRecords r;
        stream_load_records<kVec>(A.qid, A.qs, A.qe, A.tid, A.ts, A.te, first, A.n_rec, true, r);
        const unsigned rev4 = stream_load_bytes<kVec>(A.strand, first, A.n_rec);
        unsigned mask = 0;
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const IdsValid v = stream_check_ids(first + i < A.n_rec, first + i, r.q[i], r.t[i], n_reads, A.ctl);
            const bool rev = ((rev4 >> (8 * i)) & 0xFFu) != 0;
            if (v.q && v.t) {
                const unsigned dq = A.dig[r.q[i]], dt = A.dig[r.t[i]];
                const int kind = ends_kind(r.q[i], r.qs[i], r.qe[i], (int32_t)(dq & ~kBestSkipBit), r.t[i], r.ts[i], r.te[i],
                                           (int32_t)(dt & ~kBestSkipBit), rev, A.max_overhang, A.min_ratio);
                if (best_end_of(kind) >= 0) {
                    if ((dq | dt) & kBestSkipBit) tot[1] += views;
                    else mask |= (A.symmetric ? 1u : 3u) << (2 * i);
                }
            }
        }
        const long long g = first / R;
        if (first < A.n_rec) A.mask[g] = (uint8_t)mask;
        const int pc = __popc(mask);
        tot[0] += (unsigned)pc;
        const int step_total = wave_reduce_add(pc);        // (every lane of the wave is here: stream_for_each_group)
        if (lane == 0) A.step_cnt[(g - lane) / kWave] = step_total;
    });
    wave_flush_totals(tot, &A.ctl[kSgCtlViews], lane);
}

struct SgStepLoader {
    const int32_t *cnt;
    __device__ void operator()(long long i, long long (&v)[1]) const { v[0] = cnt[i]; }
};

// the items: the arcs of the views, as five columns, and the first sort's pairs (w, item index)
struct SgItems { int32_t *u, *w, *ext, *back, *span; uint32_t *key; int32_t *val; long long n; };

template <bool kVec>
__global__ __launch_bounds__(kStreamThreads) void sg_fill_kernel(SgStreamArgs A, const long long *__restrict__ step_off, SgItems out)
{
    constexpr int R = kStreamLaneRecords;
    const int lane = (int)threadIdx.x & (kWave - 1);
    stream_for_each_group(A.n_rec, lane, [&](const long long first) {
        const long long g = first / R;
        const unsigned mask = first < A.n_rec ? A.mask[g] : 0u;
        const int pc = __popc(mask);
        const int incl = wave_incl_scan_add(pc);
        long long pos = step_off[(g - lane) / kWave] + (incl - pc);
        if (mask) {
            LaneRecords r;
            stream_load_records<kVec>(A.qid, A.qs, A.qe, A.tid, A.ts, A.te, first, A.n_rec, true, r);
            const unsigned rev4 = stream_load_bytes<kVec>(A.strand, first, A.n_rec);
#pragma unroll
            for (int i = 0; i < R; ++i) {
                const unsigned m = (mask >> (2 * i)) & 3u;
                if (!m) continue;                          // (a set bit: both ids are valid, the kind is a dovetail, no side is flagged)
                const bool rev = ((rev4 >> (8 * i)) & 0xFFu) != 0;
                const int32_t lq = (int32_t)(A.dig[r.q[i]] & ~kBestSkipBit), lt = (int32_t)(A.dig[r.t[i]] & ~kBestSkipBit);
                const int kind = ends_kind(r.q[i], r.qs[i], r.qe[i], lq, r.t[i], r.ts[i], r.te[i], lt, rev, A.max_overhang, A.min_ratio);
                // the query view's arc, then -- where its bit is set -- the target view's: one arc in registers at a time
                SgArc a;
                const auto put = [&](const SgArc &x) {
                    if (pos < out.n) {                     // (always: the offsets count the same bits)
                        out.u[pos] = x.u; out.w[pos] = x.w; out.ext[pos] = x.ext; out.back[pos] = x.back; out.span[pos] = x.span;
                        out.key[pos] = (uint32_t)x.w; out.val[pos] = (int32_t)pos;
                    }
                    pos += 1;
                };
                if (!sg_view_arc(kind, r.q[i], r.qs[i], r.qe[i], lq, r.t[i], r.ts[i], r.te[i], lt, rev, &a)) continue;
                put(a);
                if ((m & 2u) && sg_view_arc(ends_target_view(kind, rev), r.t[i], r.ts[i], r.te[i], lt, r.q[i], r.qs[i], r.qe[i], lq, rev, &a)) put(a);
            }
        }
    });
}

// the second sort's keys: u of the item that the first pass left at place i
__global__ __launch_bounds__(kSgThreads) void sg_rekey_kernel(const int32_t *__restrict__ val, const int32_t *__restrict__ item_u, long long n, uint32_t *__restrict__ key)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) key[i] = (uint32_t)item_u[val[i]];
}

// key / val: the items in (u, w) order (key is u).  head[i]: item i opens a run of one (u, w); chosen[i]: the run's item with the greatest key.
__global__ __launch_bounds__(kSgThreads) void sg_choose_kernel(const uint32_t *__restrict__ key, const int32_t *__restrict__ val, SgItems it,
                                                               uint8_t *__restrict__ head, int32_t *__restrict__ chosen)
{
    const long long stride = (long long)gridDim.x * blockDim.x, n = it.n;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t u = key[i];
        int32_t best = val[i];
        const int32_t w = it.w[best];
        const bool is_head = i == 0 || key[i - 1] != u || it.w[val[i - 1]] != w;
        if (is_head) {
            SgKey bk = sg_key((int32_t)u, w, it.ext[best], it.back[best], it.span[best]);
            for (long long j = i + 1; j < n && key[j] == u; ++j) {
                const int32_t x = val[j];
                if (it.w[x] != w) break;
                const SgKey k = sg_key((int32_t)u, w, it.ext[x], it.back[x], it.span[x]);
                if (sg_key_wins(k, bk)) { bk = k; best = x; }
            }
        }
        head[i] = is_head ? 1 : 0;
        chosen[i] = best;
    }
}

struct SgByteLoader {
    const uint8_t *b; unsigned bit;
    __device__ void operator()(long long i, long long (&v)[1]) const { v[0] = (b[i] & bit) ? 1 : 0; }
};

// the chosen arcs in (u, w) order: five columns of n_arcs entries
struct SgArcs { int32_t *u, *w, *ext, *back, *span; };

__global__ __launch_bounds__(kSgThreads) void sg_compact_kernel(const uint32_t *__restrict__ key, const uint8_t *__restrict__ head, const int32_t *__restrict__ chosen,
                                                                const long long *__restrict__ pos, SgItems it, SgArcs out)
{
    const long long stride = (long long)gridDim.x * blockDim.x, n = it.n;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        if (!head[i]) continue;
        const long long p = pos[i];
        const int32_t x = chosen[i];
        out.u[p] = (int32_t)key[i]; out.w[p] = it.w[x]; out.ext[p] = it.ext[x]; out.back[p] = it.back[x]; out.span[p] = it.span[x];
    }
}

// the first place in a[lo, hi) (ascending) that holds x or more
__device__ __forceinline__ long long sg_lower_bound(const int32_t *__restrict__ a, long long lo, long long hi, int32_t x)
{
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// row[x], x = 0 .. n_nodes: where the arcs of node x begin (row[n_nodes] = n_arcs); *n_arcs is the head scan's total
__global__ __launch_bounds__(kSgThreads) void sg_rows_kernel(const int32_t *__restrict__ arc_u, const long long *__restrict__ n_arcs_p, long long n_nodes,
                                                             int32_t *__restrict__ row)
{
    const long long stride = (long long)gridDim.x * blockDim.x, n_arcs = *n_arcs_p;
    for (long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x; x <= n_nodes; x += stride)
        row[x] = x == n_nodes ? (int32_t)n_arcs : (int32_t)sg_lower_bound(arc_u, 0, n_arcs, (int32_t)x);
}

// the arc of node `from`'s row that goes to `to`, or -1
__device__ __forceinline__ long long sg_find(const int32_t *__restrict__ row, const int32_t *__restrict__ arc_w, int32_t from, int32_t to)
{
    const long long lo = row[from], hi = row[from + 1];
    const long long p = sg_lower_bound(arc_w, lo, hi, to);
    return p < hi && arc_w[p] == to ? p : -1;
}

// One wave per workgroup.  red[a] = 1 for every reducible arc a (red is zeroed before the launch).
__global__ __launch_bounds__(kWave) void sg_reduce_kernel(const int32_t *__restrict__ row, const int32_t *__restrict__ arc_w, const int32_t *__restrict__ arc_ext,
                                                          long long n_nodes, int32_t fuzz, uint8_t *__restrict__ red)
{
    __shared__ int32_t s_w[kSgRowLds], s_x[kSgRowLds];
    const int lane = (int)threadIdx.x;
    const long long n_chunks = (n_nodes + kWave - 1) / kWave;
    for (long long chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const long long x = chunk * kWave + lane;
        const int32_t r0 = row[x < n_nodes ? x : n_nodes], r1 = row[x + 1 < n_nodes ? x + 1 : n_nodes];
        const int32_t len = x < n_nodes ? r1 - r0 : 0;
        unsigned long long todo = __ballot(len >= 2);      // (a row of one arc has no via)
        while (todo) {
            const int b = (int)__builtin_ctzll(todo);
            todo &= todo - 1;
            const long long s = __shfl(r0, b, kWave), L = __shfl(len, b, kWave);
            const bool in_lds = L <= kSgRowLds;
            __syncthreads();                               // (one wave: the row before has been read)
            if (in_lds)
                for (long long k = lane; k < L; k += kWave) { s_w[k] = arc_w[s + k]; s_x[k] = arc_ext[s + k]; }
            __syncthreads();
            const long long pairs = L * L;
            for (long long p = lane; p < pairs; p += kWave) {
                const long long a = p / L, via = p - a * L;
                if (a == via) continue;
                const int32_t ext_uw = in_lds ? s_x[a] : arc_ext[s + a], ext_uv = in_lds ? s_x[via] : arc_ext[s + via];
                if (!(ext_uv < ext_uw)) continue;
                const int32_t w = in_lds ? s_w[a] : arc_w[s + a], v = in_lds ? s_w[via] : arc_w[s + via];
                const long long t = sg_find(row, arc_w, v ^ 1, w);
                if (t >= 0 && sg_reducible(ext_uv, arc_ext[t], ext_uw, fuzz)) red[s + a] = 1;
            }
        }
    }
}

// state[a] of every arc: its own flag, its twin's, whether it has one, whether its edge survives and whether it is listed
__global__ __launch_bounds__(kSgThreads) void sg_pair_kernel(const int32_t *__restrict__ row, SgArcs arc, const long long *__restrict__ n_arcs_p,
                                                             const uint8_t *__restrict__ red, int32_t emit_removed, uint8_t *__restrict__ state,
                                                             unsigned long long *__restrict__ ctl)
{
    const long long stride = (long long)gridDim.x * blockDim.x, n_arcs = *n_arcs_p;
    const int lane = (int)threadIdx.x & (kWave - 1);
    unsigned tot[4] = {0, 0, 0, 0};                        // unpaired, reducible, edges, kept edges
    for (long long a0 = (long long)blockIdx.x * blockDim.x + ((int)threadIdx.x & ~(kWave - 1)); a0 < n_arcs; a0 += stride) {
        const long long a = a0 + lane;
        if (a < n_arcs) {
            const int32_t u = arc.u[a], w = arc.w[a];
            const long long t = sg_find(row, arc.w, w, u);
            const bool mine = red[a] != 0, theirs = t >= 0 && red[t] != 0, unpaired = t < 0;
            const bool survives = !mine && !theirs, is_edge = unpaired || (u >> 1) < (w >> 1);
            const bool listed = is_edge && (emit_removed || survives);
            state[a] = (uint8_t)((mine ? kSgStRed : 0u) | (theirs ? kSgStTwinRed : 0u) | (unpaired ? kSgStUnpaired : 0u) | (survives ? kSgStSurvives : 0u) |
                                 (listed ? kSgStListed : 0u));
            tot[0] += unpaired ? 1u : 0u; tot[1] += mine ? 1u : 0u; tot[2] += is_edge ? 1u : 0u; tot[3] += (is_edge && survives) ? 1u : 0u;
        }
    }
    wave_flush_totals(tot, &ctl[kSgCtlUnpaired], lane);    // (all lanes are back together here)
}

// per node: the row's length, the arcs of it whose edge survives, and that arc where it is the only one (-1 otherwise)
__global__ __launch_bounds__(kSgThreads) void sg_ends_kernel(const int32_t *__restrict__ row, const uint8_t *__restrict__ state, long long n_nodes,
                                                             int32_t *__restrict__ n_arcs, int32_t *__restrict__ kept, int32_t *__restrict__ sole)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x; x < n_nodes; x += stride) {
        const int32_t lo = row[x], hi = row[x + 1];
        int32_t k = 0, last = -1;
        for (int32_t a = lo; a < hi; ++a)
            if (state[a] & kSgStSurvives) { k += 1; last = a; }
        n_arcs[x] = hi - lo; kept[x] = k; sole[x] = k == 1 ? last : -1;
    }
}

__device__ __forceinline__ unsigned sg_wave_max(unsigned v)
{
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) {
        const unsigned o = __shfl_xor(v, d, kWave);
        v = o > v ? o : v;
    }
    return v;
}

// per read: the unitig table (partner, span of both ends, the flag byte) and the totals over the ends
__global__ __launch_bounds__(kSgThreads) void sg_table_kernel(const unsigned *__restrict__ dig, int32_t n_reads, SgArcs arc, const uint8_t *__restrict__ state,
                                                              const int32_t *__restrict__ n_arcs, const int32_t *__restrict__ kept, const int32_t *__restrict__ sole,
                                                              int32_t *__restrict__ partner, int32_t *__restrict__ span, uint8_t *__restrict__ flags,
                                                              unsigned long long *__restrict__ ctl)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    const int lane = (int)threadIdx.x & (kWave - 1);
    unsigned tot[kSgEndTotals] = {};                       // ends_with_arc, kept_one, kept_more, mutual, dead, reads_flagged
    unsigned longest = 0;
    for (long long r0 = (long long)blockIdx.x * blockDim.x + ((int)threadIdx.x & ~(kWave - 1)); r0 < n_reads; r0 += stride) {
        const long long r = r0 + lane;
        if (r < n_reads) {
            const bool skipped = (dig[r] & kBestSkipBit) != 0;
            unsigned flag = skipped ? (unsigned)kBestSkipped : 0u;
            int p[2] = {-1, -1}, s[2] = {0, 0};
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int32_t u = (int32_t)(2 * r + e);
                const int32_t len = n_arcs[u], k = kept[u];
                tot[0] += len > 0 ? 1u : 0u; tot[1] += k == 1 ? 1u : 0u; tot[2] += k >= 2 ? 1u : 0u; tot[4] += (!skipped && k == 0) ? 1u : 0u;
                longest = (unsigned)len > longest ? (unsigned)len : longest;
                if (k != 1) continue;
                const int32_t a = sole[u];
                const int32_t w = arc.w[a];
                if ((state[a] & kSgStUnpaired) || kept[w] != 1) continue;
                const int32_t t = sole[w];
                if (arc.w[t] != u || arc.span[t] != arc.span[a]) continue;
                p[e] = w >> 1; s[e] = arc.span[a];
                flag |= (((w & 1) == e ? (unsigned)kBestRev5 : 0u) | (unsigned)kBestMutual5) << (2 * e);
                tot[3] += 1;
            }
            *reinterpret_cast<int2 *>(partner + 2 * r) = make_int2(p[0], p[1]);
            *reinterpret_cast<int2 *>(span + 2 * r) = make_int2(s[0], s[1]);
            flags[r] = (uint8_t)flag;
            tot[5] += skipped ? 1u : 0u;
        }
    }
    wave_flush_totals(tot, &ctl[kSgCtlEnds], lane);        // (all lanes are back together here)
    const unsigned m = sg_wave_max(longest);
    if (lane == 0 && m) atomicMax(&ctl[kSgCtlLongest], (unsigned long long)m);
}

struct SgEdges { int32_t *u, *w, *span, *ext, *back; uint8_t *flags; };

__global__ __launch_bounds__(kSgThreads) void sg_edges_kernel(SgArcs arc, const long long *__restrict__ n_arcs_p, const uint8_t *__restrict__ state,
                                                              const long long *__restrict__ pos, SgEdges out)
{
    const long long stride = (long long)gridDim.x * blockDim.x, n_arcs = *n_arcs_p;
    for (long long a = (long long)blockIdx.x * blockDim.x + threadIdx.x; a < n_arcs; a += stride) {
        const unsigned st = state[a];
        if (!(st & kSgStListed)) continue;
        const long long p = pos[a];
        out.u[p] = arc.u[a]; out.w[p] = arc.w[a]; out.span[p] = arc.span[a]; out.ext[p] = arc.ext[a]; out.back[p] = arc.back[a];
        out.flags[p] = (uint8_t)(st & (kSgStRed | kSgStTwinRed | kSgStUnpaired));
    }
}

} // namespace raft
