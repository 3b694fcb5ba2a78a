// ovl_ends.hpp -- which end of each read every record supports (raft_hip_overlap_ends_device / _host, include/raft_hip_end.h): the
// kind of every record under the rule of ovl_ends_rule.hpp, per read the five counts, the status bytes, the totals.
//
// One streaming kernel of record_stream.hpp's shape: the six columns and the lane's four strand bytes (25 B per record in); it
// gathers the two lengths of every record, evaluates the rule and stores the lane's four kind bytes as one 32-bit word when the
// caller wants them (strand and kinds are byte columns: the vector path needs them on a 4-byte line).
//   * counts: a record adds 1 to one of five counts of its query's row and, unless symmetric, of its target's.  join_runs joins equal
//     neighbouring ids before the adds -- in ONE segmented scan over the five partial counts held in 12-bit fields of a 64-bit word
//     (a run within a wave has at most 256 records), not one scan per count: six steps of three shuffles where five scans take
//     sixty.  What leaves is one add per run, wave and count that is not 0.  The target column takes the same route, joining what
//     happens to be equal.
//   * an id outside [0, n_reads) in either column: the first bad record is kept, the record is counted nowhere.
//   * the kind totals are kept per lane and leave with one atomic per wave (wave_flush_totals) when the wave has no more records.
// A second kernel over the reads makes the status bytes and the status totals.  No workgroup waits for another.
#pragma once
#include "record_stream.hpp"
#include "ovl_ends_rule.hpp"

namespace raft {

constexpr int kEndsFieldBits = 12;           // a count's field in the joined word: 5 * 12 bits, each holding up to 4095
// control words: the first bad record, the records by kind, the reads by status
constexpr int kEndsCtlKinds = 1, kEndsCtlStatus = kEndsCtlKinds + kEndKinds, kEndsCtlWords = kEndsCtlStatus + kEndStatuses;
static_assert(kStreamWaveRecords < (1 << kEndsFieldBits), "a run within a wave fits a field");

struct EndsArgs {
    const int32_t *len, *qid, *qs, *qe, *tid, *ts, *te;
    const uint8_t *strand;
    uint8_t *kinds;                          // may be NULL
    long long n_rec;
    int32_t n_reads, max_overhang, min_ratio, symmetric;
    unsigned *cnt;                           // [kEndCounts * n_reads], zeroed before the launch
    unsigned long long *ctl;                 // kEndsCtlWords
};

// the fields of a joined word that are not 0, each to its count of read `id`
__device__ __forceinline__ void ends_emit(unsigned *__restrict__ cnt, unsigned n_reads, int id, unsigned long long x)
{
#pragma unroll
    for (int k = 0; k < kEndCounts; ++k) {
        const unsigned f = (unsigned)(x >> (kEndsFieldBits * k)) & ((1u << kEndsFieldBits) - 1u);
        if (f) atomicAdd(&cnt[(size_t)k * n_reads + (unsigned)id], f);
    }
}

template <bool kVec>
__global__ __launch_bounds__(kStreamThreads) void ends_kernel(EndsArgs A)
{
    constexpr int R = kStreamLaneRecords;
    const int lane = (int)threadIdx.x & (kWave - 1);
    const unsigned n_reads = (unsigned)A.n_reads;
    // cnt[k][id] += field k of the sum of the joined words of the wave's records with that id (a word of 0 adds nothing whatever its id)
    unsigned *const cnt = A.cnt;
    const auto emit = [cnt, n_reads](int id, unsigned long long x) { if (x) ends_emit(cnt, n_reads, id, x); };
    unsigned tot[kEndKinds] = {};
    // stream_for_each_group's loop, written out: under the helper the register allocation of ends_kernel<false> comes out two VGPRs
    // higher (66), one step of occupancy below what this form gives.  As there, the loop's bound is the wave's, never the lane's:
    // every lane of a wave takes part in join_runs' shuffles (EXEC all ones).
    const long long n_groups = (A.n_rec + R - 1) / R;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long g0 = (long long)blockIdx.x * blockDim.x + ((int)threadIdx.x & ~(kWave - 1)); g0 < n_groups; g0 += stride) {
        const long long first = (g0 + lane) * R;
        LaneRecords r;
        stream_load_records<kVec>(A.qid, A.qs, A.qe, A.tid, A.ts, A.te, first, A.n_rec, true, r);
        const unsigned rev4 = stream_load_bytes<kVec>(A.strand, first, A.n_rec);
        unsigned long long wq[R], wt[R];
        unsigned kind4 = 0;
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const bool have = first + i < A.n_rec;
            const IdsValid v = stream_check_ids(have, first + i, r.q[i], r.t[i], n_reads, A.ctl);
            const bool rev = ((rev4 >> (8 * i)) & 0xFFu) != 0;
            int kind = kEndInvalid;
            if (v.q && v.t)
                kind = ends_kind(r.q[i], r.qs[i], r.qe[i], A.len[r.q[i]], r.t[i], r.ts[i], r.te[i], A.len[r.t[i]], rev, A.max_overhang, A.min_ratio);
            kind4 |= (unsigned)kind << (8 * i);
#pragma unroll
            for (int k = 0; k < kEndKinds; ++k) tot[k] += (have && kind == k) ? 1u : 0u;
            const int sq = ends_count_slot(kind), st = ends_count_slot(ends_target_view(kind, rev));
            wq[i] = sq >= 0 ? 1ull << (kEndsFieldBits * sq) : 0ull;
            wt[i] = (!A.symmetric && st >= 0) ? 1ull << (kEndsFieldBits * st) : 0ull;
        }
        if (A.kinds) stream_store_bytes<kVec>(A.kinds, first, A.n_rec, kind4);
        join_runs(r.q, wq, lane, JoinAdd{}, emit);
        if (!A.symmetric) join_runs(r.t, wt, lane, JoinAdd{}, emit);
    }
    // (all lanes of the wave are back together here)
    wave_flush_totals(tot, &A.ctl[kEndsCtlKinds], lane);
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
    wave_flush_totals(tot, &ctl[kEndsCtlStatus], lane);     // (all lanes are back together here)
}

} // namespace raft
