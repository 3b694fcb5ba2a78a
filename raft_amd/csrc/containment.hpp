// containment.hpp -- the containment forest (raft_hip_containment_device / _host) and the forest laid onto a unitig layout
// (raft_hip_place_contained_device / _host), include/raft_hip_ctn.h: two streaming passes that choose every read's parent and its
// place in it, pointer jumping over the reads up to the roots, one reduction per root.
//
// Kernels, none of which waits for another workgroup (one launch each; the host looks at the control words once, behind the last):
//   * ctn_stream_kernel<kVec, 1>: one streaming pass of record_stream.hpp's shape -- the six columns and the lane's four strand bytes,
//     the two lengths gathered, the kind under ovl_ends_rule.hpp, the record's view under containment_rule.hpp.  An acceptable view
//     brings key1 to its read's slot (join_runs under max: one atomicMax per run and wave, and only while the slot is below); any
//     other flags its read, look before atomic.  A record with an id out of range is kept as the first bad record and gives no view.
//   * ctn_stream_kernel<kVec, 2>: the same pass again -- it classifies again and reads no kind byte: a byte per record written and
//     read back is 2 B of traffic on 25 B, and the lengths it would spare are gathered for the key anyway --, decodes the parent from
//     the slot pass 1 left and brings key2 of the views that name it to the second slot.
//   * ctn_init_kernel: a lane per read: the two keys -> parent, pos, span, the flag word and the 16-byte state {anc, pos, bits,
//     depth}; children[parent] += 1.  A read whose parent is a root is finished here.
//   * ctn_jump_kernel: ceil(log2(max(n, 2))) rounds between two state buffers, one launch per round and no host wait between them:
//     an open state takes its ancestor's state (one 16-byte gather) and the ancestor's length, composes the two places and adds the
//     depths; a finished state -- its ancestor is a root -- gathers nothing and is copied.  After round k every read of depth
//     <= 2^k is finished; the last round counts the open ones, which the rule says are none.
//   * ctn_tree_kernel: four consecutive reads per lane; (1, depth, length) joined by root within the wave and added once per run and
//     wave to the root's accumulators.
//   * ctn_emit_kernel: root, root_pos, depth and the flag byte of every read; the totals kept per lane, one atomic per wave and total.
//   * ctn_place_kernel / ctn_depth_kernel: the second call -- every read through its root onto the root's unitig, (1, contained,
//     length) joined by unitig within the wave; then a lane per unitig.
#pragma once
#include "record_stream.hpp"
#include "containment_rule.hpp"

namespace raft {

constexpr int kCtnThreads = 256;
constexpr int kCtnMaxBlocks = 2048;          // eight workgroups on each of the 256 CUs, grid-stride beyond
// control words of the first call: the first bad record, the views, the views not longer, the open states, then ctn_emit_kernel's
// totals -- four sums, three maxima
constexpr int kCtnCtlViews = 1, kCtnCtlNotLonger = 2, kCtnCtlOpen = 3, kCtnCtlTotals = 4;
constexpr int kCtnWithParent = 0, kCtnOrphans = 1, kCtnRoots = 2, kCtnRootsWithTree = 3, kCtnGreatestDepth = 4, kCtnLargestReads = 5, kCtnLargestBases = 6;
constexpr int kCtnTotals = 7, kCtnCtlWords = kCtnCtlTotals + kCtnTotals;
// ... of the second: the first bad read, the placed reads, the unitigs that gained a read, the greatest depth
constexpr int kPlcCtlPlaced = 1, kPlcCtlGained = 2, kPlcCtlGreatest = 3, kPlcCtlWords = 4;

inline unsigned ctn_grid(long long n) { return (unsigned)(n < 1 ? 1 : ((n + kCtnThreads - 1) / kCtnThreads > kCtnMaxBlocks ? kCtnMaxBlocks : (n + kCtnThreads - 1) / kCtnThreads)); }

__device__ __forceinline__ long long ctn_len(int32_t len) { return len > 0 ? len : 0; }

// slot = max(slot, key).  A read's views are neighbours in the stream and most of them lose: the slot is looked at first and the atomic
// goes out only while it is below.  Slots only ever rise, so a stale look costs an atomic, never a key.
__device__ __forceinline__ void ctn_raise(unsigned long long *slot, unsigned long long key)
{
    if (__atomic_load_n(slot, __ATOMIC_RELAXED) < key) atomicMax(slot, key);
}

struct JoinMax {
    template <class V> __device__ __forceinline__ V operator()(V a, V b) const { return a > b ? a : b; }
};

struct CtnStreamArgs {
    const int32_t *len, *qid, *qs, *qe, *tid, *ts, *te;
    const uint8_t *strand;
    long long n_rec;
    int32_t n_reads, max_overhang, min_ratio, symmetric;
    unsigned long long *key1, *key2;         // [n_reads] each, zeroed
    unsigned *flagw;                         // [n_reads], zeroed
    unsigned long long *ctl;                 // kCtnCtlWords
};

template <bool kVec, int kPass>
__global__ __launch_bounds__(kStreamThreads) void ctn_stream_kernel(CtnStreamArgs A)
{
    constexpr int R = kStreamLaneRecords;
    const int lane = (int)threadIdx.x & (kWave - 1);
    const unsigned n_reads = (unsigned)A.n_reads;
    unsigned long long *const slot = kPass == 1 ? A.key1 : A.key2;
    // slot[id] = max(slot[id], the greatest key of the wave's run with that id) (0 brings nothing whatever the id)
    const auto emit = [slot](int id, unsigned long long x) { if (x) ctn_raise(&slot[(unsigned)id], x); };
    unsigned tot[2] = {0, 0};                // views, views not longer (pass 1)
    stream_for_each_group(A.n_rec, lane, [&](long long first) {
        LaneRecords r;
        stream_load_records<kVec>(A.qid, A.qs, A.qe, A.tid, A.ts, A.te, first, A.n_rec, true, r);
        const unsigned rev4 = stream_load_bytes<kVec>(A.strand, first, A.n_rec);
        unsigned long long wq[R], wt[R];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const bool have = first + i < A.n_rec;
            // (pass 1 keeps the first bad record; pass 2 only needs to know which ids it may gather by)
            const IdsValid v = kPass == 1 ? stream_check_ids(have, first + i, r.q[i], r.t[i], n_reads, A.ctl)
                                          : IdsValid{have && (unsigned)r.q[i] < n_reads, have && (unsigned)r.t[i] < n_reads};
            const bool rev = ((rev4 >> (8 * i)) & 0xFFu) != 0;
            int kind = kEndInvalid;
            int32_t lq = 0, lt = 0;
            if (v.q && v.t) {
                lq = A.len[r.q[i]]; lt = A.len[r.t[i]];
                kind = ends_kind(r.q[i], r.qs[i], r.qe[i], lq, r.t[i], r.ts[i], r.te[i], lt, rev, A.max_overhang, A.min_ratio);
            }
            wq[i] = 0; wt[i] = 0;
            const bool from_query = kind == kEndQueryContained, from_target = kind == kEndTargetContained && !A.symmetric;
            if (from_query || from_target) {               // (a record gives one view at the most)
                const CtnView w = from_query ? ctn_query_view(r.q[i], r.qs[i], r.qe[i], r.t[i], r.ts[i], r.te[i])
                                             : ctn_target_view(r.q[i], r.qs[i], r.qe[i], r.t[i], r.ts[i], r.te[i]);
                const int32_t lr = from_query ? lq : lt, lc = from_query ? lt : lq;
                const bool ok = ctn_acceptable(lr, w.r, lc, w.c);
                unsigned long long key = 0;
                if (kPass == 1) {
                    tot[0] += 1;
                    if (ok) key = ctn_key1(lc, w.c);
                    else { tot[1] += 1; ovl_flag(&A.flagw[w.r], kCtnUnplacedView); }
                } else if (ok && ctn_key1_parent(A.key1[w.r]) == w.c) key = ctn_view_key2(w, lr, lc, rev);
                if (from_query) wq[i] = key; else wt[i] = key;
            }
        }
        // (all lanes of the wave are back together here)
        join_runs(r.q, wq, lane, JoinMax{}, emit);
        if (!A.symmetric) join_runs(r.t, wt, lane, JoinMax{}, emit);
    });
    if (kPass == 1) wave_flush_totals(tot, &A.ctl[kCtnCtlViews], lane);
}

// A read on its way to the root: it lies in `anc` at `pos`, reversed iff bit 0 of `bits`, `depth` containers below it; bit 1 of
// `bits`: anc is a root, the state is finished.  A root is {itself, 0, finished, 0}.  One 16-byte line: one load, one store.
struct alignas(16) CtnState { int32_t anc, pos; uint32_t bits; int32_t depth; };
constexpr uint32_t kCtnStateRev = 1, kCtnStateDone = 2;

__device__ __forceinline__ CtnState ctn_load_state(const CtnState *s)
{
    const int4 q = *reinterpret_cast<const int4 *>(s);
    return CtnState{q.x, q.y, (uint32_t)q.z, q.w};
}
__device__ __forceinline__ void ctn_store_state(CtnState *s, CtnState v)
{
    *reinterpret_cast<int4 *>(s) = make_int4(v.anc, v.pos, (int)v.bits, v.depth);
}

struct CtnInitOut { int32_t *parent, *pos, *span; };

__global__ __launch_bounds__(kCtnThreads) void ctn_init_kernel(int32_t n_reads, const unsigned long long *__restrict__ key1,
                                                               const unsigned long long *__restrict__ key2, unsigned *__restrict__ flagw,
                                                               unsigned *__restrict__ children, CtnState *__restrict__ state, CtnInitOut out)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += stride) {
        const int32_t par = ctn_key1_parent(key1[r]);
        unsigned f = flagw[r] & kCtnUnplacedView;
        if (par < 0 || (unsigned)par >= (unsigned)n_reads) {           // (a key names a read of a record with two valid ids: the second never holds)
            ctn_store_state(state + r, CtnState{(int32_t)r, 0, kCtnStateDone, 0});
            out.parent[r] = -1; out.pos[r] = 0; out.span[r] = 0;
            if (f) f |= kCtnOrphan;
        } else {
            const unsigned long long k2 = key2[r];
            const bool rev = ctn_key2_rev(k2);
            const int32_t pos = ctn_key2_pos(k2);
            const bool done = key1[par] == 0;                          // the parent is a root
            ctn_store_state(state + r, CtnState{par, pos, (rev ? kCtnStateRev : 0u) | (done ? kCtnStateDone : 0u), 1});
            out.parent[r] = par; out.pos[r] = pos; out.span[r] = ctn_key2_span(k2);
            atomicAdd(&children[(unsigned)par], 1u);
            f |= kCtnHasParent | (rev ? kCtnParentRev : 0u);
        }
        flagw[r] = f;
    }
}

// One round: dst[r] = src[r] composed with src[src[r].anc] where src[r] is open.  src is read-only in this launch.
template <bool kLast>
__global__ __launch_bounds__(kCtnThreads) void ctn_jump_kernel(int32_t n_reads, const int32_t *__restrict__ len, const CtnState *__restrict__ src,
                                                               CtnState *__restrict__ dst, unsigned long long *__restrict__ ctl)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    const int lane = (int)threadIdx.x & (kWave - 1);
    unsigned open[1] = {0};
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += stride) {
        CtnState s = ctn_load_state(src + r);
        if (!(s.bits & kCtnStateDone) && (unsigned)s.anc < (unsigned)n_reads) {
            const CtnState a = ctn_load_state(src + s.anc);
            const CtnPlace p = ctn_compose(CtnPlace{s.pos, (s.bits & kCtnStateRev) != 0}, len[r], len[s.anc], CtnPlace{a.pos, (a.bits & kCtnStateRev) != 0});
            s = CtnState{a.anc, p.pos, (p.rev ? kCtnStateRev : 0u) | (a.bits & kCtnStateDone), s.depth + a.depth};
        }
        ctn_store_state(dst + r, s);
        if (kLast && !(s.bits & kCtnStateDone)) open[0] += 1;
    }
    // (all lanes are back together here)
    if (kLast) wave_flush_totals(open, &ctl[kCtnCtlOpen], lane);
}

// the per-root accumulators: bases [n], then reads [n] and depth [n]; they are the outputs tree_bases, tree_reads and tree_depth
struct CtnAcc { unsigned long long *bases; unsigned *reads, *depth; };

// the value of ctn_tree_kernel's join: what the reads of a run bring to their root; three shuffles
struct CtnSum { unsigned reads, depth; unsigned long long bases; };

__device__ __forceinline__ CtnSum join_shfl_up(CtnSum v, int d) { return CtnSum{join_shfl_up(v.reads, d), join_shfl_up(v.depth, d), join_shfl_up(v.bases, d)}; }

struct CtnSumJoin {
    __device__ __forceinline__ CtnSum operator()(CtnSum a, CtnSum b) const { return CtnSum{a.reads + b.reads, a.depth > b.depth ? a.depth : b.depth, a.bases + b.bases}; }
};

__global__ __launch_bounds__(kStreamThreads) void ctn_tree_kernel(const CtnState *__restrict__ state, const int32_t *__restrict__ len, int32_t n_reads, CtnAcc acc)
{
    constexpr int R = kStreamLaneRecords;
    const int lane = (int)threadIdx.x & (kWave - 1);
    // (a root, and a read behind n_reads, come with the id -1 and bring nothing: emit looks at the value first)
    const auto emit = [acc](int id, CtnSum x) {
        if (!x.reads) return;
        atomicAdd(&acc.reads[(unsigned)id], x.reads);
        atomicMax(&acc.depth[(unsigned)id], x.depth);
        if (x.bases) atomicAdd(&acc.bases[(unsigned)id], x.bases);
    };
    stream_for_each_group((long long)n_reads, lane, [&](long long first) {
        int id[R];
        CtnSum w[R];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const long long r = first + i;
            id[i] = -1; w[i] = CtnSum{0u, 0u, 0ull};
            if (r < n_reads) {
                const CtnState s = ctn_load_state(state + r);
                if (s.depth > 0 && (unsigned)s.anc < (unsigned)n_reads) { id[i] = s.anc; w[i] = CtnSum{1u, (unsigned)s.depth, (unsigned long long)ctn_len(len[r])}; }
            }
        }
        join_runs(id, w, lane, CtnSumJoin{}, emit);
    });
}

__device__ __forceinline__ long long ctn_wave_max(long long v)
{
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) {
        const long long o = __shfl_xor(v, d, kWave);
        v = o > v ? o : v;
    }
    return v;
}

struct CtnEmitOut { int32_t *root, *root_pos, *depth; uint8_t *flags; };

__global__ __launch_bounds__(kCtnThreads) void ctn_emit_kernel(const CtnState *__restrict__ state, const unsigned *__restrict__ flagw, int32_t n_reads,
                                                               CtnAcc acc, CtnEmitOut out, unsigned long long *__restrict__ ctl)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    const int lane = (int)threadIdx.x & (kWave - 1);
    unsigned counts[4] = {0, 0, 0, 0};                     // with a parent, orphans, roots, roots with a tree
    long long greatest = 0, largest_reads = 0, largest_bases = 0;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += stride) {
        const CtnState s = ctn_load_state(state + r);
        const unsigned f = flagw[r] | ((s.bits & kCtnStateRev) ? kCtnRootRev : 0u);
        out.root[r] = s.anc; out.root_pos[r] = s.pos; out.depth[r] = s.depth; out.flags[r] = (uint8_t)f;
        counts[kCtnWithParent] += s.depth > 0 ? 1u : 0u;
        counts[kCtnOrphans] += (f & kCtnOrphan) ? 1u : 0u;
        if (s.depth == 0) {
            const long long reads = acc.reads[r], bases = (long long)acc.bases[r];
            counts[kCtnRoots] += 1; counts[kCtnRootsWithTree] += reads > 0 ? 1u : 0u;
            largest_reads = reads > largest_reads ? reads : largest_reads;
            largest_bases = bases > largest_bases ? bases : largest_bases;
        }
        greatest = s.depth > greatest ? s.depth : greatest;
    }
    // (all lanes are back together here)
    const unsigned long long mine = wave_lane_totals(counts, lane);
    const long long gd = ctn_wave_max(greatest), lr = ctn_wave_max(largest_reads), lb = ctn_wave_max(largest_bases);
    if (lane < kCtnGreatestDepth) { if (mine) atomicAdd(&ctl[kCtnCtlTotals + lane], mine); }
    else if (lane == kCtnGreatestDepth) { if (gd) atomicMax(&ctl[kCtnCtlTotals + lane], (unsigned long long)gd); }
    else if (lane == kCtnLargestReads) { if (lr) atomicMax(&ctl[kCtnCtlTotals + lane], (unsigned long long)lr); }
    else if (lane == kCtnLargestBases) { if (lb) atomicMax(&ctl[kCtnCtlTotals + lane], (unsigned long long)lb); }
}

// ---- the second call
// the per-unitig accumulators: bases [U], then reads [U] and contained [U]; the first two are the outputs placed_bases and placed_reads
struct PlcAcc { unsigned long long *bases; unsigned *reads, *contained; };

struct PlcArgs {
    int32_t n_reads, n_unitigs;
    const int32_t *len, *root, *root_pos;
    const uint8_t *flags;
    const int32_t *unitig;
    const long long *offset;
    const uint8_t *orient;
    int32_t *placed_unitig; long long *start; uint8_t *placed_orient;      // [n_reads] each
    PlcAcc acc;                              // zeroed
    unsigned long long *ctl;                 // kPlcCtlWords
};

// (reads, bases) as CtnSum has them; `depth` holds the reads with a parent, and is added
struct PlcSumJoin {
    __device__ __forceinline__ CtnSum operator()(CtnSum a, CtnSum b) const { return CtnSum{a.reads + b.reads, a.depth + b.depth, a.bases + b.bases}; }
};

__global__ __launch_bounds__(kStreamThreads) void ctn_place_kernel(PlcArgs A)
{
    constexpr int R = kStreamLaneRecords;
    const int lane = (int)threadIdx.x & (kWave - 1);
    const PlcAcc acc = A.acc;
    const auto emit = [acc](int id, CtnSum x) {
        if (!x.reads) return;
        atomicAdd(&acc.reads[(unsigned)id], x.reads);
        if (x.depth) atomicAdd(&acc.contained[(unsigned)id], x.depth);
        if (x.bases) atomicAdd(&acc.bases[(unsigned)id], x.bases);
    };
    unsigned placed[1] = {0};
    stream_for_each_group((long long)A.n_reads, lane, [&](long long first) {
        int id[R];
        CtnSum w[R];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const long long r = first + i;
            id[i] = -1; w[i] = CtnSum{0u, 0u, 0ull};
            if (r >= A.n_reads) continue;
            const int32_t own = A.unitig[r], top = A.root[r];
            const bool top_ok = (unsigned)top < (unsigned)A.n_reads;
            if (!top_ok || own < -1 || own >= A.n_unitigs) atomicMin(A.ctl, (unsigned long long)r);
            int32_t u = -1;
            long long start = 0;
            unsigned o = 0;
            // (the root's own unitig id is checked by the root's lane: out of range it places nobody here)
            if (top_ok) { const int32_t ut = A.unitig[top]; if (ut >= 0 && ut < A.n_unitigs) u = ut; }
            if (u >= 0) {
                const bool to = A.orient[top] != 0;
                start = ctn_unitig_start(A.offset[top], to, A.len[top], A.root_pos[r], A.len[r]);
                o = (to ? 1u : 0u) ^ ((A.flags[r] & kCtnRootRev) ? 1u : 0u);
                id[i] = u; w[i] = CtnSum{1u, top != (int32_t)r ? 1u : 0u, (unsigned long long)ctn_len(A.len[r])};
                placed[0] += 1;
            }
            A.placed_unitig[r] = u; A.start[r] = start; A.placed_orient[r] = (uint8_t)o;
        }
        join_runs(id, w, lane, PlcSumJoin{}, emit);
    });
    wave_flush_totals(placed, &A.ctl[kPlcCtlPlaced], lane);
}

__global__ __launch_bounds__(kCtnThreads) void ctn_depth_kernel(int32_t n_unitigs, const long long *__restrict__ utg_length, PlcAcc acc,
                                                                long long *__restrict__ depth_permille, unsigned long long *__restrict__ ctl)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    const int lane = (int)threadIdx.x & (kWave - 1);
    unsigned gained[1] = {0};
    long long greatest = 0;
    for (long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x; u < n_unitigs; u += stride) {
        const long long d = ctn_depth_permille((long long)acc.bases[u], utg_length[u]);
        depth_permille[u] = d;
        gained[0] += acc.contained[u] > 0 ? 1u : 0u;
        greatest = d > greatest ? d : greatest;
    }
    // (all lanes are back together here)
    const unsigned long long mine = wave_lane_totals(gained, lane);
    const long long g = ctn_wave_max(greatest);
    if (lane == 0) {
        if (mine) atomicAdd(&ctl[kPlcCtlGained], mine);
        if (g) atomicMax(&ctl[kPlcCtlGreatest], (unsigned long long)g);
    }
}

} // namespace raft
