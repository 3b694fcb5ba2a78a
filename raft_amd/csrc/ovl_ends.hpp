// ovl_ends.hpp -- which end of each read every record supports (raft_hip_overlap_ends_device / _host, include/raft_hip_end.h): the
// kind of every record under the rule of ovl_ends_rule.hpp, per read the five counts, the status bytes, the totals.
//
// One streaming kernel of the census's shape (census.hpp): a lane takes kCensusLaneRecords consecutive records per step, the six
// columns with census_load's 16-byte loads and the lane's four strand bytes with one 32-bit load (25 B per record in); it gathers
// the two lengths of every record, evaluates the rule and stores the lane's four kind bytes as one 32-bit word when the caller
// wants them.  Columns that do not begin on a 16-byte line (strand, kinds: on a 4-byte one), and the records behind the last whole
// group, take element loads and stores.
//   * counts: a record adds 1 to one of five counts of its query's row and, unless symmetric, of its target's.  The query column is
//     mostly sorted runs, so equal neighbouring ids are joined before the adds, as census_count does -- but in ONE segmented scan over
//     the five partial counts held in 12-bit fields of a 64-bit word (a run within a wave has at most 256 records), not one scan per
//     count: six steps of three shuffles where five scans take sixty.  What leaves is one add per run, wave and count that is not 0.
//     The target column takes the same route, joining what happens to be equal.
//   * an id outside [0, n_reads) in either column: the smallest such record index is kept (atomicMin), the record is counted nowhere.
//   * the kind totals are kept per lane and leave with one atomic per wave (lane k adds kind k) when the wave has no more records.
// A second kernel over the reads makes the status bytes and the status totals.  No workgroup waits for another.
#pragma once
#include "census.hpp"
#include "ovl_ends_rule.hpp"

namespace raft {

constexpr int kEndsThreads = 256;
constexpr int kEndsMaxBlocks = 2048;         // eight workgroups on each of the 256 CUs, grid-stride beyond
constexpr int kEndsFieldBits = 12;           // a count's field in the joined word: 5 * 12 bits, each holding up to 4095
// control words: the first bad record, the records by kind, the reads by status
constexpr int kEndsCtlKinds = 1, kEndsCtlStatus = kEndsCtlKinds + kEndKinds, kEndsCtlWords = kEndsCtlStatus + kEndStatuses;
static_assert(kWave * kCensusLaneRecords < (1 << kEndsFieldBits), "a run within a wave fits a field");

struct EndsArgs {
    const int32_t *len, *qid, *qs, *qe, *tid, *ts, *te;
    const uint8_t *strand;
    uint8_t *kinds;                          // may be NULL
    long long n_rec;
    int32_t n_reads, max_overhang, min_ratio, symmetric;
    unsigned *cnt;                           // [kEndCounts * n_reads], zeroed before the launch
    unsigned long long *ctl;                 // kEndsCtlWords
};

inline unsigned ends_grid(long long n_rec)
{
    const long long per_step = (long long)kEndsThreads * kCensusLaneRecords;         // records one workgroup takes per step
    const long long want = (n_rec + per_step - 1) / per_step;
    return (unsigned)(want < 1 ? 1 : (want > kEndsMaxBlocks ? kEndsMaxBlocks : want));
}

// the fields of a joined word that are not 0, each to its count of read `id`
__device__ __forceinline__ void ends_emit(unsigned *__restrict__ cnt, unsigned n_reads, int id, unsigned long long x)
{
#pragma unroll
    for (int k = 0; k < kEndCounts; ++k) {
        const unsigned f = (unsigned)(x >> (kEndsFieldBits * k)) & ((1u << kEndsFieldBits) - 1u);
        if (f) atomicAdd(&cnt[(size_t)k * n_reads + (unsigned)id], f);
    }
}

// census_count over joined words: cnt[k][id] += field k of the sum of w over the lane's records with that id, for every lane of the
// wave.  A record with w = 0 adds nothing whatever its id (ids out of range come with w = 0).  EXEC must be all ones.
__device__ __forceinline__ void ends_count(const int (&id)[kCensusLaneRecords], const unsigned long long (&w)[kCensusLaneRecords],
                                           unsigned *__restrict__ cnt, unsigned n_reads, int lane)
{
    int cur = id[0];
    unsigned long long n = w[0], head_n = 0;
    bool uniform = true;
#pragma unroll
    for (int i = 1; i < kCensusLaneRecords; ++i) {
        if (id[i] == cur) n += w[i];
        else {
            if (uniform) { head_n = n; uniform = false; }
            else if (n) ends_emit(cnt, n_reads, cur, n);   // a run that touches neither end of the lane
            cur = id[i]; n = w[i];
        }
    }
    // the lane's last run (cur, n) opens a segment unless the lane is one run that carries on what the lane before ended with
    const int prev_tail = __shfl_up(cur, 1, kWave);
    const bool joins = lane > 0 && id[0] == prev_tail;
    unsigned long long x = n;
    int f = (!uniform || !joins) ? 1 : 0;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const unsigned long long xo = __shfl_up(x, d, kWave);
        const int fo = __shfl_up(f, d, kWave);
        if (lane >= d && !f) { x += xo; f = fo; }
    }
    const unsigned long long before = __shfl_up(x, 1, kWave);        // the open run as the lane before left it
    const int next_joins = __shfl_down(joins ? 1 : 0, 1, kWave);
    if (!uniform) {
        const unsigned long long h = head_n + (joins ? before : 0ull);
        if (h) ends_emit(cnt, n_reads, id[0], h);
    }
    if ((lane == kWave - 1 || !next_joins) && x) ends_emit(cnt, n_reads, cur, x);
}

template <bool kVec>
__global__ __launch_bounds__(kEndsThreads) void ends_kernel(EndsArgs A)
{
    constexpr int R = kCensusLaneRecords;
    static_assert(R == 4, "four strand bytes, four kind bytes: one word");
    const int lane = (int)threadIdx.x & (kWave - 1);
    const long long n_groups = (A.n_rec + R - 1) / R;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const unsigned n_reads = (unsigned)A.n_reads;
    unsigned tot[kEndKinds] = {};
    // (the loop's bound is the wave's: every lane of a wave takes part in the scans)
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
        unsigned long long wq[R], wt[R];
        unsigned kind4 = 0;
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const bool have = first + i < A.n_rec;
            const bool vq = have && (unsigned)q[i] < n_reads, vt = have && (unsigned)t[i] < n_reads;
            if (have && !(vq && vt)) atomicMin(A.ctl, (unsigned long long)(first + i));
            const bool rev = ((rev4 >> (8 * i)) & 0xFFu) != 0;
            int kind = kEndInvalid;
            if (vq && vt) kind = ends_kind(q[i], qs[i], qe[i], A.len[q[i]], t[i], ts[i], te[i], A.len[t[i]], rev, A.max_overhang, A.min_ratio);
            kind4 |= (unsigned)kind << (8 * i);
#pragma unroll
            for (int k = 0; k < kEndKinds; ++k) tot[k] += (have && kind == k) ? 1u : 0u;
            const int sq = ends_count_slot(kind), st = ends_count_slot(ends_target_view(kind, rev));
            wq[i] = sq >= 0 ? 1ull << (kEndsFieldBits * sq) : 0ull;
            wt[i] = (!A.symmetric && st >= 0) ? 1ull << (kEndsFieldBits * st) : 0ull;
        }
        if (A.kinds) {
            if (whole) *reinterpret_cast<unsigned *>(A.kinds + first) = kind4;
            else {
#pragma unroll
                for (int i = 0; i < R; ++i)
                    if (first + i < A.n_rec) A.kinds[first + i] = (uint8_t)(kind4 >> (8 * i));
            }
        }
        ends_count(q, wq, A.cnt, n_reads, lane);
        if (!A.symmetric) ends_count(t, wt, A.cnt, n_reads, lane);
    }
    // (all lanes of the wave are back together here) lane k holds the wave's records of kind k
    unsigned mine = 0;
#pragma unroll
    for (int k = 0; k < kEndKinds; ++k) {
        const unsigned total = (unsigned)wave_reduce_add((int)tot[k]);
        if (lane == k) mine = total;
    }
    if (lane < kEndKinds && mine) atomicAdd(&A.ctl[kEndsCtlKinds + lane], (unsigned long long)mine);
}

// the counts of every read -> its status byte, and the reads by status
__global__ __launch_bounds__(256) void ends_status_kernel(const unsigned *__restrict__ cnt, int32_t n_reads, uint8_t *__restrict__ status,
                                                          unsigned long long *__restrict__ ctl)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    const int lane = (int)threadIdx.x & (kWave - 1);
    unsigned tot[kEndStatuses] = {};
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += stride) {
        const int s = ends_status((int32_t)cnt[(size_t)1 * n_reads + r], (int32_t)cnt[(size_t)3 * n_reads + r], (int32_t)cnt[(size_t)4 * n_reads + r]);
        status[r] = (uint8_t)s;
#pragma unroll
        for (int k = 0; k < kEndStatuses; ++k) tot[k] += s == k ? 1u : 0u;
    }
    unsigned mine = 0;                                     // (all lanes are back together here)
#pragma unroll
    for (int k = 0; k < kEndStatuses; ++k) {
        const unsigned total = (unsigned)wave_reduce_add((int)tot[k]);
        if (lane == k) mine = total;
    }
    if (lane < kEndStatuses && mine) atomicAdd(&ctl[kEndsCtlStatus + lane], (unsigned long long)mine);
}

} // namespace raft
