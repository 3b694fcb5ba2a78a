// components.hpp -- the connected components of the overlap graph (raft_hip_components_device / _host, include/raft_hip_cc.h): a
// concurrent union over the edge records of a stream, then one pass per read that turns the forest into dense component ids.
//
// Kernels, none of which waits for another workgroup (one launch each; the host looks at the control words once, behind the last):
//   * cc_init_kernel: parent[r] = r, degree[r] = 0, the per-root accumulators 0.
//   * cc_link_kernel: one streaming pass of record_stream.hpp's shape -- the six columns and the lane's four strand bytes (25 B per
//     record in), the two lengths gathered, the kind under ovl_ends_rule.hpp, the mask.  An edge record adds 1 to its query's degree
//     and, unless symmetric, to its target's (join_runs: one add per run and wave), and its two reads are united (cc_unite below).
//     A record with an id out of range is kept as the first bad record and links nothing.
//   * cc_flatten_kernel: a lane per read walks `parent` to its root and writes root[r]; parent is read-only in this launch.
//   * cc_sum_kernel: four consecutive reads per lane; (1, length, degree) joined by root within the wave (neighbouring reads of a
//     large component share their root) and added once per run and wave to the root's accumulators.
//   * one exclusive scan (device_scan.hpp) over "read r is a root": the dense ids in the order of the smallest read ids.
//   * cc_emit_kernel: component[r] = prefix[root[r]]; a root writes its component's row; the totals are kept per lane and leave
//     with one atomic per wave and total.
#pragma once
#include "record_stream.hpp"
#include "ovl_ends_rule.hpp"

#ifndef RAFT_CC_HALVE
#define RAFT_CC_HALVE 1                      // path halving in cc_unite's walks (profiles/components_timing.txt)
#endif

namespace raft {

constexpr int kCcThreads = 256;
constexpr int kCcMaxBlocks = 2048;           // eight workgroups on each of the 256 CUs, grid-stride beyond
constexpr bool kCcHalve = RAFT_CC_HALVE != 0;
constexpr int kCcKindBits = 0x3E;            // the kinds 1 .. 5: what a mask may hold
// control words: the first bad record, the edge records, then the totals of cc_emit_kernel
constexpr int kCcCtlEdges = 1, kCcCtlTotals = 2;
constexpr int kCcComponents = 0, kCcSingletons = 1, kCcTotalBases = 2, kCcLargestReads = 3, kCcLargestBases = 4;
constexpr int kCcTotals = 5, kCcCtlWords = kCcCtlTotals + kCcTotals;

inline unsigned cc_grid(long long n) { return (unsigned)(n < 1 ? 1 : ((n + kCcThreads - 1) / kCcThreads > kCcMaxBlocks ? kCcMaxBlocks : (n + kCcThreads - 1) / kCcThreads)); }

__device__ __forceinline__ long long cc_len(int32_t len) { return len > 0 ? len : 0; }

// the per-root accumulators: reads [n], then bases [n] and sides [n]
struct CcAcc { unsigned *reads; unsigned long long *bases, *sides; };

__global__ __launch_bounds__(kCcThreads) void cc_init_kernel(int32_t n_reads, int32_t *__restrict__ parent, unsigned *__restrict__ degree, CcAcc acc)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += stride) {
        parent[r] = (int32_t)r; degree[r] = 0;
        acc.reads[r] = 0; acc.bases[r] = 0; acc.sides[r] = 0;
    }
}

// parent[x] as some workgroup left it: a relaxed load at agent scope (it does not stop at this CU's L1)
__device__ __forceinline__ int32_t cc_parent(const int32_t *parent, int32_t x)
{
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Unites the trees of reads a and b: a lock-free union-find that links by id.  What it rests on:
//   1. parent[x] <= x always, and parent[x] < x once x is not a root.  Every write keeps it: the init writes x; the one write that turns
//      a root into a non-root is atomicCAS(&parent[hi], hi, lo) with lo < hi, which succeeds only while hi is a root -- so a read stops
//      being a root once, and never becomes one again; halving writes onto a non-root x an ancestor of x, which is below x.  Hence no
//      cycles, every tree's root is its smallest read, and since a record's two reads end in one tree and a tree only ever holds reads
//      that records connect, the trees at the end of the launch are the components whatever the order of the records and however the
//      workgroups were scheduled.
//   2. A stale read of parent[x] is harmless.  The L2s of the XCDs are not coherent with each other, so a load may return a value
//      parent[x] held earlier.  Every value parent[x] ever held is x itself or an ancestor of x -- and stays one: an ancestor's own
//      link upwards is never taken back, only replaced by a link further up.  A stale "x is a root" makes the CAS fail, and the CAS
//      returns the value that is there, from which the walk goes on; a stale "lo is a root" links hi under a read that is no root
//      but has a smaller id and lies in the tree hi is meant to join.  Both keep (1).  The loads are relaxed agent-scope atomic
//      loads, the CAS is at device scope (atomicCAS's default): it is served where every XCD's atomics are.
//   3. Every step descends: it replaces the larger of the two reads by its parent, or the smaller by its, each strictly smaller, or it
//      ends the walk -- at most a + b steps.  No lane waits for a value somebody else must write: no spin, no look-back.
//   4. Look before you write: when the two walks meet, a == b, the reads are joined already and no atomic goes out.  In a sorted run
//      of one query id most records arrive that way.
// Halving (kHalve): a step from a non-root x over p = parent[x] looks at parent[p] as well and, where p is no root either, stores it
// into parent[x] -- a relaxed agent-scope atomic store of a value read from x's chain onto a read seen as a non-root, which no CAS
// can ever succeed on again.  Two such stores may land in either order: either value is an ancestor of x.
template <bool kHalve>
__device__ __forceinline__ void cc_unite(int32_t *parent, int32_t a, int32_t b)
{
    while (a != b) {
        if (a < b) { const int32_t t = a; a = b; b = t; }  // a: the larger
        const int32_t pa = cc_parent(parent, a);
        if (pa != a) {                                     // a is no root: a step up its chain
            if (kHalve && pa != b) {
                const int32_t ga = cc_parent(parent, pa);
                if (ga != pa) __hip_atomic_store(parent + a, ga, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                a = ga;                                    // (pa where pa is a root: parent[pa] == pa)
            } else a = pa;
            continue;
        }
        const int32_t pb = cc_parent(parent, b);
        if (pb != b) { b = pb; continue; }                 // the smaller is no root yet: a step up its chain
        const int32_t was = atomicCAS(parent + a, a, b);   // both seen as roots: the larger under the smaller
        if (was == a) return;
        a = was;                                           // somebody else linked a first: on from where it hangs now
    }
}

struct CcLinkArgs {
    const int32_t *len, *qid, *qs, *qe, *tid, *ts, *te;
    const uint8_t *strand;
    long long n_rec;
    int32_t n_reads, max_overhang, min_ratio, kind_mask, symmetric;
    int32_t *parent;                         // [n_reads], cc_init_kernel's
    unsigned *degree;                        // [n_reads], zeroed
    unsigned long long *ctl;                 // kCcCtlWords
};

template <bool kVec, bool kHalve>
__global__ __launch_bounds__(kStreamThreads) void cc_link_kernel(CcLinkArgs A)
{
    constexpr int R = kStreamLaneRecords;
    const int lane = (int)threadIdx.x & (kWave - 1);
    const unsigned n_reads = (unsigned)A.n_reads;
    unsigned *const degree = A.degree;
    // degree[id] += the edge records of the wave's run with that id (0 adds nothing whatever the id)
    const auto emit = [degree](int id, unsigned x) { if (x) atomicAdd(&degree[(unsigned)id], x); };
    unsigned tot[1] = {0};
    stream_for_each_group(A.n_rec, lane, [&](long long first) {
        LaneRecords r;
        stream_load_records<kVec>(A.qid, A.qs, A.qe, A.tid, A.ts, A.te, first, A.n_rec, true, r);
        const unsigned rev4 = stream_load_bytes<kVec>(A.strand, first, A.n_rec);
        unsigned wq[R], wt[R];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const bool have = first + i < A.n_rec;
            const IdsValid v = stream_check_ids(have, first + i, r.q[i], r.t[i], n_reads, A.ctl);
            const bool rev = ((rev4 >> (8 * i)) & 0xFFu) != 0;
            int kind = kEndInvalid;
            if (v.q && v.t)
                kind = ends_kind(r.q[i], r.qs[i], r.qe[i], A.len[r.q[i]], r.t[i], r.ts[i], r.te[i], A.len[r.t[i]], rev, A.max_overhang, A.min_ratio);
            const bool edge = ((A.kind_mask >> kind) & 1) != 0;      // (the mask holds neither 0 nor 6: no edge without two valid ids)
            tot[0] += edge ? 1u : 0u;
            wq[i] = edge ? 1u : 0u;
            wt[i] = (edge && !A.symmetric) ? 1u : 0u;
            if (edge) cc_unite<kHalve>(A.parent, r.q[i], r.t[i]);
        }
        // (all lanes of the wave are back together here)
        join_runs(r.q, wq, lane, JoinAdd{}, emit);
        if (!A.symmetric) join_runs(r.t, wt, lane, JoinAdd{}, emit);
    });
    wave_flush_totals(tot, &A.ctl[kCcCtlEdges], lane);
}

// root[r]: the end of r's chain.  parent is not written in this launch, and the launch boundary made every link visible.
__global__ __launch_bounds__(kCcThreads) void cc_flatten_kernel(const int32_t *__restrict__ parent, int32_t n_reads, int32_t *__restrict__ root)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += stride) {
        int32_t x = (int32_t)r, p = parent[x];
        while (p != x) { x = p; p = parent[x]; }           // (descends: parent[x] < x for every non-root)
        root[r] = x;
    }
}

// the value of cc_sum_kernel's join: what the reads of a run bring to their root; three shuffles
struct CcSum { unsigned reads; unsigned long long bases, sides; };

__device__ __forceinline__ CcSum join_shfl_up(CcSum v, int d) { return CcSum{join_shfl_up(v.reads, d), join_shfl_up(v.bases, d), join_shfl_up(v.sides, d)}; }

struct CcSumAdd {
    __device__ __forceinline__ CcSum operator()(CcSum a, CcSum b) const { return CcSum{a.reads + b.reads, a.bases + b.bases, a.sides + b.sides}; }
};

__global__ __launch_bounds__(kStreamThreads) void cc_sum_kernel(const int32_t *__restrict__ root, const int32_t *__restrict__ len,
                                                                const unsigned *__restrict__ degree, int32_t n_reads, CcAcc acc)
{
    constexpr int R = kStreamLaneRecords;
    const int lane = (int)threadIdx.x & (kWave - 1);
    // (a read behind n_reads comes with the id -1 and brings nothing: emit looks at the value first)
    const auto emit = [acc](int id, CcSum x) {
        if (!x.reads) return;
        atomicAdd(&acc.reads[(unsigned)id], x.reads);
        if (x.bases) atomicAdd(&acc.bases[(unsigned)id], x.bases);
        if (x.sides) atomicAdd(&acc.sides[(unsigned)id], x.sides);
    };
    stream_for_each_group((long long)n_reads, lane, [&](long long first) {
        int id[R];
        CcSum w[R];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const long long r = first + i;
            const bool have = r < n_reads;
            id[i] = have ? root[r] : -1;
            w[i] = have ? CcSum{1u, (unsigned long long)cc_len(len[r]), (unsigned long long)degree[r]} : CcSum{0u, 0ull, 0ull};
        }
        join_runs(id, w, lane, CcSumAdd{}, emit);
    });
}

// the scan's element: read i is a root
struct CcRootLoader {
    const int32_t *root;
    __device__ void operator()(long long i, long long (&v)[1]) const { v[0] = root[i] == (int32_t)i ? 1 : 0; }
};

__device__ __forceinline__ long long cc_wave_max(long long v)
{
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) {
        const long long o = __shfl_xor(v, d, kWave);
        v = o > v ? o : v;
    }
    return v;
}

struct CcOut {
    int32_t *component;                      // [n_reads]
    int32_t *first, *reads; long long *bases, *sides;      // [n_reads] each, C entries written
};

__global__ __launch_bounds__(kCcThreads) void cc_emit_kernel(const int32_t *__restrict__ root, int32_t n_reads, const long long *__restrict__ root_id,
                                                             CcAcc acc, CcOut out, unsigned long long *__restrict__ ctl)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    const int lane = (int)threadIdx.x & (kWave - 1);
    unsigned counts[2] = {0, 0};                           // components, singletons
    long long total_bases = 0, largest_reads = 0, largest_bases = 0;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += stride) {
        const int32_t top = root[r];
        const long long c = root_id[top];
        out.component[r] = (int32_t)c;
        if (top == (int32_t)r) {
            const long long reads = acc.reads[r], bases = (long long)acc.bases[r];
            out.first[c] = (int32_t)r; out.reads[c] = (int32_t)reads; out.bases[c] = bases; out.sides[c] = (long long)acc.sides[r];
            counts[kCcComponents] += 1; counts[kCcSingletons] += reads == 1 ? 1u : 0u;
            total_bases += bases;
            largest_reads = reads > largest_reads ? reads : largest_reads;
            largest_bases = bases > largest_bases ? bases : largest_bases;
        }
    }
    // (all lanes are back together here)
    unsigned long long mine = wave_lane_totals(counts, lane);
    const long long tb = wave_reduce_add64(total_bases), lr = cc_wave_max(largest_reads), lb = cc_wave_max(largest_bases);
    if (lane == kCcTotalBases) mine = (unsigned long long)tb;
    if (lane < kCcLargestReads) { if (mine) atomicAdd(&ctl[kCcCtlTotals + lane], mine); }
    else if (lane == kCcLargestReads) { if (lr) atomicMax(&ctl[kCcCtlTotals + lane], (unsigned long long)lr); }
    else if (lane == kCcLargestBases) { if (lb) atomicMax(&ctl[kCcCtlTotals + lane], (unsigned long long)lb); }
}

} // namespace raft
