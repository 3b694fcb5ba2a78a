// best_ovl.hpp -- the best overlap of every read end (raft_hip_best_overlaps_device / _host, include/raft_hip_best.h): per read and
// end the greatest key of best_ovl_rule.hpp among the dovetail views whose two reads are not left out, whether the choice is mutual,
// the totals.
//
// Three kernels, none of which waits for another workgroup:
//   * best_digest_kernel: len | (skip != 0) << 31 per read in one 32-bit word, so that the stream gathers one word per id and not a
//     length and a byte.  (A length below 0 becomes 0: no record on such a read is valid, as under ends_kind.)
//   * best_kernel<kVec>, of the census's shape (census.hpp), reading the stream exactly as ends_kernel does: four consecutive
//     records per lane, the six columns with census_load's 16-byte loads, the lane's four strand bytes with one 32-bit load (25 B per
//     record in), element loads for columns off the line and for the records behind the last whole group.  It evaluates ends_kind
//     and reduces the candidates' keys into a uint64 [2 * n_reads] table, cleared before every launch.
//       - query side: the column is mostly sorted runs, so equal neighbouring ids are joined before anything leaves the wave -- a
//         segmented MAX scan over the lanes' last runs that carries the 5' and the 3' maximum, of ends_count's structure with max
//         where that has add.  What leaves is at most one 64-bit atomicMax per run, wave and end, and only for a key that is not 0.
//       - target side: the column is random and only a dovetail between two reads that are not left out has a key, so nothing is
//         joined: each key goes to its slot directly, behind a relaxed load of the slot that skips a key which cannot win (the
//         table only grows within a launch, so a stale value is a smaller one and skips less, never wrongly).
//       - an id outside [0, n_reads) in either column: the smallest such record index is kept (atomicMin), the record has no view.
//       - candidates and left_out are kept per lane and leave with one atomic per wave (lane 0 the first, lane 1 the second).
//   * best_pairs_kernel: one lane per read handles both of its slots -- it unpacks them, reads the two partner slots for mutuality,
//     writes partner and span (one 8-byte store each) and the flag byte (one plain store: no two lanes share a byte); the read
//     totals are kept per lane and leave with one atomic per wave.
#pragma once
#include "census.hpp"
#include "best_ovl_rule.hpp"

namespace raft {

constexpr int kBestThreads = 256;
constexpr int kBestMaxBlocks = 2048;         // eight workgroups on each of the 256 CUs, grid-stride beyond
// control words: the first bad record, {candidates, left_out}, the six read totals
constexpr int kBestCtlViews = 1, kBestCtlReads = 3, kBestReadTotals = 6, kBestCtlWords = kBestCtlReads + kBestReadTotals;
constexpr unsigned kBestSkipBit = 0x80000000u;

struct BestArgs {
    const unsigned *dig;                     // [n_reads]: len | skipped << 31
    const int32_t *qid, *qs, *qe, *tid, *ts, *te;
    const uint8_t *strand;
    long long n_rec;
    int32_t n_reads, max_overhang, min_ratio, symmetric;
    unsigned long long *tab;                 // [2 * n_reads], zeroed before the launch
    unsigned long long *ctl;                 // kBestCtlWords
};

inline unsigned best_grid(long long n_rec)
{
    const long long per_step = (long long)kBestThreads * kCensusLaneRecords;         // records one workgroup takes per step
    const long long want = (n_rec + per_step - 1) / per_step;
    return (unsigned)(want < 1 ? 1 : (want > kBestMaxBlocks ? kBestMaxBlocks : want));
}

__global__ __launch_bounds__(256) void best_digest_kernel(const int32_t *__restrict__ len, const uint8_t *__restrict__ skip, int32_t n_reads,
                                                          unsigned *__restrict__ dig)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += stride) {
        const int32_t l = len[r];
        dig[r] = (l < 0 ? 0u : (unsigned)l) | ((skip && skip[r]) ? kBestSkipBit : 0u);
    }
}

__device__ __forceinline__ unsigned long long best_max(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

// the two maxima of a run to the slots of read `id` (a key of 0 is no candidate and goes nowhere)
__device__ __forceinline__ void best_emit(unsigned long long *__restrict__ tab, int id, unsigned long long k5, unsigned long long k3)
{
    if (k5) atomicMax(&tab[2 * (size_t)(unsigned)id], k5);
    if (k3) atomicMax(&tab[2 * (size_t)(unsigned)id + 1], k3);
}

// ends_count with max for add, over two values: tab[2 * id + E] = max(itself, the greatest k<E> of the lane's records with that id),
// for every lane of the wave.  A record with both keys 0 changes nothing whatever its id (ids out of range come with keys 0).
// EXEC must be all ones.
__device__ __forceinline__ void best_reduce(const int (&id)[kCensusLaneRecords], const unsigned long long (&k5)[kCensusLaneRecords],
                                            const unsigned long long (&k3)[kCensusLaneRecords], unsigned long long *__restrict__ tab, int lane)
{
    int cur = id[0];
    unsigned long long a = k5[0], b = k3[0], head_a = 0, head_b = 0;
    bool uniform = true;
#pragma unroll
    for (int i = 1; i < kCensusLaneRecords; ++i) {
        if (id[i] == cur) { a = best_max(a, k5[i]); b = best_max(b, k3[i]); }
        else {
            if (uniform) { head_a = a; head_b = b; uniform = false; }
            else best_emit(tab, cur, a, b);                // a run that touches neither end of the lane
            cur = id[i]; a = k5[i]; b = k3[i];
        }
    }
    // the lane's last run (cur, a, b) opens a segment unless the lane is one run that carries on what the lane before ended with
    const int prev_tail = __shfl_up(cur, 1, kWave);
    const bool joins = lane > 0 && id[0] == prev_tail;
    unsigned long long x = a, y = b;
    int f = (!uniform || !joins) ? 1 : 0;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const unsigned long long xo = __shfl_up(x, d, kWave), yo = __shfl_up(y, d, kWave);
        const int fo = __shfl_up(f, d, kWave);
        if (lane >= d && !f) { x = best_max(x, xo); y = best_max(y, yo); f = fo; }
    }
    const unsigned long long before_x = __shfl_up(x, 1, kWave), before_y = __shfl_up(y, 1, kWave);   // the open run as the lane before left it
    const int next_joins = __shfl_down(joins ? 1 : 0, 1, kWave);
    if (!uniform) best_emit(tab, id[0], joins ? best_max(head_a, before_x) : head_a, joins ? best_max(head_b, before_y) : head_b);
    if (lane == kWave - 1 || !next_joins) best_emit(tab, cur, x, y);
}

template <bool kVec>
__global__ __launch_bounds__(kBestThreads) void best_kernel(BestArgs A)
{
    constexpr int R = kCensusLaneRecords;
    static_assert(R == 4, "four strand bytes: one word");
    const int lane = (int)threadIdx.x & (kWave - 1);
    const long long n_groups = (A.n_rec + R - 1) / R;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const unsigned n_reads = (unsigned)A.n_reads;
    const unsigned views = A.symmetric ? 1u : 2u;
    unsigned cand = 0, left = 0;
    // (the loop's bound is the wave's: every lane of a wave takes part in the scan)
    for (long long g0 = (long long)blockIdx.x * blockDim.x + ((int)threadIdx.x & ~(kWave - 1)); g0 < n_groups; g0 += stride) {
        const long long first = (g0 + lane) * R;           // (at or beyond n_rec: a lane without records)
        const bool whole = kVec && first + R <= A.n_rec;
        int q[R], t[R], qs[R], qe[R], ts[R], te[R];
        census_load<kVec>(A.qid, first, A.n_rec, -1, q);
        census_load<kVec>(A.tid, first, A.n_rec, -1, t);
        census_load<kVec>(A.qs, first, A.n_rec, -1, qs);
        census_load<kVec>(A.qe, first, A.n_rec, -1, qe);
        census_load<kVec>(A.ts, first, A.n_rec, -1, ts);
        census_load<kVec>(A.te, first, A.n_rec, -1, te);
        unsigned rev4 = 0;
        if (whole) rev4 = *reinterpret_cast<const unsigned *>(A.strand + first);
        else {
#pragma unroll
            for (int i = 0; i < R; ++i)
                if (first + i < A.n_rec) rev4 |= (unsigned)A.strand[first + i] << (8 * i);
        }
        unsigned long long k5[R], k3[R];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const bool have = first + i < A.n_rec;
            const bool vq = have && (unsigned)q[i] < n_reads, vt = have && (unsigned)t[i] < n_reads;
            if (have && !(vq && vt)) atomicMin(A.ctl, (unsigned long long)(first + i));
            const bool rev = ((rev4 >> (8 * i)) & 0xFFu) != 0;
            k5[i] = 0; k3[i] = 0;
            if (vq && vt) {
                const unsigned dq = A.dig[q[i]], dt = A.dig[t[i]];
                const int kind = ends_kind(q[i], qs[i], qe[i], (int32_t)(dq & ~kBestSkipBit), t[i], ts[i], te[i], (int32_t)(dt & ~kBestSkipBit), rev,
                                           A.max_overhang, A.min_ratio);
                const int eq = best_end_of(kind);
                if (eq >= 0) {
                    if ((dq | dt) & kBestSkipBit) left += views;
                    else {
                        cand += views;
                        const int32_t span = qe[i] - qs[i] < te[i] - ts[i] ? qe[i] - qs[i] : te[i] - ts[i];
                        const unsigned long long kq = best_pack(span, t[i], rev);
                        if (eq == 0) k5[i] = kq; else k3[i] = kq;
                        if (!A.symmetric) {
                            const unsigned long long kt = best_pack(span, q[i], rev);
                            unsigned long long *slot = &A.tab[2 * (size_t)(unsigned)t[i] + (unsigned)best_end_of(ends_target_view(kind, rev))];
                            if (__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < kt) atomicMax(slot, kt);
                        }
                    }
                }
            }
        }
        best_reduce(q, k5, k3, A.tab, lane);
    }
    // (all lanes of the wave are back together here)
    const unsigned c = (unsigned)wave_reduce_add((int)cand), l = (unsigned)wave_reduce_add((int)left);
    const unsigned mine = lane == 0 ? c : l;
    if (lane < 2 && mine) atomicAdd(&A.ctl[kBestCtlViews + lane], (unsigned long long)mine);
}

// the slots of every read -> partner, span, the flag byte; the read totals: ends_best, ends_mutual, reads_both_best,
// reads_both_mutual, reads_no_best, reads_skipped
__global__ __launch_bounds__(256) void best_pairs_kernel(const unsigned long long *__restrict__ tab, const unsigned *__restrict__ dig, int32_t n_reads,
                                                         int32_t *__restrict__ partner, int32_t *__restrict__ span, uint8_t *__restrict__ flags,
                                                         unsigned long long *__restrict__ ctl)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    const int lane = (int)threadIdx.x & (kWave - 1);
    unsigned tot[kBestReadTotals] = {};
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += stride) {
        const ulonglong2 mine = *reinterpret_cast<const ulonglong2 *>(tab + 2 * r);
        const unsigned long long key[2] = {mine.x, mine.y};
        const bool skipped = (dig[r] & kBestSkipBit) != 0;
        int p[2], s[2];
        unsigned flag = skipped ? (unsigned)kBestSkipped : 0u, n_best = 0, n_mutual = 0;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            p[e] = -1; s[e] = 0;
            if (key[e]) {
                p[e] = best_partner(key[e]); s[e] = best_span(key[e]);
                const bool rev = best_rev(key[e]);
                const unsigned long long theirs = tab[2 * (size_t)p[e] + (unsigned)best_partner_end(e, rev)];
                const bool mutual = best_mutual((int32_t)r, e, key[e], theirs);
                flag |= (rev ? (unsigned)kBestRev5 : 0u) << (2 * e) | (mutual ? (unsigned)kBestMutual5 : 0u) << (2 * e);
                n_best += 1; n_mutual += mutual ? 1u : 0u;
            }
        }
        *reinterpret_cast<int2 *>(partner + 2 * r) = make_int2(p[0], p[1]);
        *reinterpret_cast<int2 *>(span + 2 * r) = make_int2(s[0], s[1]);
        flags[r] = (uint8_t)flag;
        tot[0] += n_best; tot[1] += n_mutual;
        tot[2] += n_best == 2 ? 1u : 0u; tot[3] += n_mutual == 2 ? 1u : 0u;
        tot[4] += (!skipped && n_best == 0) ? 1u : 0u; tot[5] += skipped ? 1u : 0u;
    }
    unsigned mine = 0;                                     // (all lanes are back together here)
#pragma unroll
    for (int k = 0; k < kBestReadTotals; ++k) {
        const unsigned total = (unsigned)wave_reduce_add((int)tot[k]);
        if (lane == k) mine = total;
    }
    if (lane < kBestReadTotals && mine) atomicAdd(&ctl[kBestCtlReads + lane], (unsigned long long)mine);
}

} // namespace raft
