// census.hpp -- what a record stream says about each read (raft_hip_census_device / _host), independent of any pass:
//
//     intervals[r] = intervals the pass piles up on read r: one per record with qid == r and, unless symmetric, one per record with
//                    tid == r and tid != qid (chop.hpp:165-169 with repeat.hpp:48-58)
//     flags[r]     = bit 0: some record has qid == r, qs == 0, qe == len[r] and len[tid] > len[r]
//                    bit 1 (not symmetric only): some record has tid == r, ts == 0, te == len[r] and len[qid] > len[r]
//
// The columns are streamed once with 16-byte loads, kCensusLaneRecords consecutive records per lane (16 B per record when symmetric,
// 24 otherwise); a stream whose columns are not 16-byte aligned, and the records behind the last whole group, take 4-byte loads.
//   * containment looks at qs == 0 (ts == 0) before it gathers any length: the two random reads of read_len happen for the few
//     candidates only, and the flag goes out with an atomic OR on the read's own word;
//   * counts: a stream is mostly sorted runs of one query id, so one global atomic per record would queue up on one address.  Equal
//     neighbouring ids are joined within the lane and then across the wave (a segmented scan over the lanes' last runs: a lane
//     whose records are all on the read the lane before ended with carries that run on), and one add goes out per run and wave.
//     The target column takes the same route with weight 0 for a record on its query's own read.
//   * an id outside [0, n_reads) in either column: the smallest such record index is kept (atomicMin) and nothing is counted for
//     that side.
#pragma once
#include "raft_types.hpp"
#include "wave.hpp"

namespace raft {

constexpr int kCensusThreads = 256;
constexpr int kCensusLaneRecords = 4;        // consecutive records of one lane per step: one 16-byte load per column
constexpr int kCensusMaxBlocks = 2048;       // eight workgroups on each of the 256 CUs, grid-stride beyond

struct CensusArgs {
    const int32_t *len, *qid, *qs, *qe, *tid, *ts, *te;
    long long n_rec;
    int32_t n_reads, symmetric;
    unsigned *intervals, *flags;             // [n_reads] each, zeroed before the launch
    unsigned long long *err;                 // smallest record index with an id out of range; ~0 = none
};

inline unsigned census_grid(long long n_rec)
{
    const long long per_step = (long long)kCensusThreads * kCensusLaneRecords;       // records one workgroup takes per step
    const long long want = (n_rec + per_step - 1) / per_step;
    return (unsigned)(want < 1 ? 1 : (want > kCensusMaxBlocks ? kCensusMaxBlocks : want));
}

template <bool kVec>
__device__ __forceinline__ void census_load(const int32_t *col, long long first, long long n_rec, int fill, int (&v)[kCensusLaneRecords])
{
    if (kVec && first + kCensusLaneRecords <= n_rec) {
        const int4 q = *reinterpret_cast<const int4 *>(col + first);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int i = 0; i < kCensusLaneRecords; ++i) v[i] = first + i < n_rec ? col[first + i] : fill;
    }
}

// cnt[id] += sum of w over the lane's records with that id, for every lane of the wave: equal neighbours are joined first.  A record
// with w = 0 adds nothing whatever its id (ids out of range come with w = 0).  EXEC must be all ones.
__device__ __forceinline__ void census_count(const int (&id)[kCensusLaneRecords], const unsigned (&w)[kCensusLaneRecords], unsigned *__restrict__ cnt, int lane)
{
    int cur = id[0];
    unsigned n = w[0], head_n = 0;
    bool uniform = true;
#pragma unroll
    for (int i = 1; i < kCensusLaneRecords; ++i) {
        if (id[i] == cur) n += w[i];
        else {
            if (uniform) { head_n = n; uniform = false; }
            else if (n) atomicAdd(&cnt[cur], n);           // a run that touches neither end of the lane
            cur = id[i]; n = w[i];
        }
    }
    // the lane's last run (cur, n) opens a segment unless the lane is one run that carries on what the lane before ended with
    const int prev_tail = __shfl_up(cur, 1, kWave);
    const bool joins = lane > 0 && id[0] == prev_tail;
    unsigned x = n;
    int f = (!uniform || !joins) ? 1 : 0;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const unsigned xo = __shfl_up(x, d, kWave);
        const int fo = __shfl_up(f, d, kWave);
        if (lane >= d && !f) { x += xo; f = fo; }
    }
    const unsigned before = __shfl_up(x, 1, kWave);        // the open run as the lane before left it
    const int next_joins = __shfl_down(joins ? 1 : 0, 1, kWave);
    if (!uniform) {
        const unsigned h = head_n + (joins ? before : 0u);
        if (h) atomicAdd(&cnt[id[0]], h);
    }
    if ((lane == kWave - 1 || !next_joins) && x) atomicAdd(&cnt[cur], x);
}

template <bool kVec>
__global__ __launch_bounds__(kCensusThreads) void census_kernel(CensusArgs A)
{
    constexpr int R = kCensusLaneRecords;
    const int lane = (int)threadIdx.x & (kWave - 1);
    const long long n_groups = (A.n_rec + R - 1) / R;
    const long long stride = (long long)gridDim.x * blockDim.x;
    const unsigned n_reads = (unsigned)A.n_reads;
    // (the loop's bound is the wave's: every lane of a wave takes part in the scans)
    for (long long g0 = (long long)blockIdx.x * blockDim.x + ((int)threadIdx.x & ~(kWave - 1)); g0 < n_groups; g0 += stride) {
        const long long first = (g0 + lane) * R;           // (at or beyond n_rec: a lane without records)
        int q[R], t[R], a[R], b[R];
        census_load<kVec>(A.qid, first, A.n_rec, -1, q);
        census_load<kVec>(A.tid, first, A.n_rec, -1, t);
        census_load<kVec>(A.qs, first, A.n_rec, -1, a);
        census_load<kVec>(A.qe, first, A.n_rec, -1, b);
        unsigned wq[R], wt[R];
        bool both[R];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const bool have = first + i < A.n_rec;
            const bool vq = have && (unsigned)q[i] < n_reads, vt = have && (unsigned)t[i] < n_reads;
            if (have && !(vq && vt)) atomicMin(A.err, (unsigned long long)(first + i));
            wq[i] = vq ? 1u : 0u;
            wt[i] = (!A.symmetric && vt && t[i] != q[i]) ? 1u : 0u;
            both[i] = vq && vt;
            if (both[i] && a[i] == 0) {
                const int lq = A.len[q[i]];
                if (b[i] == lq && A.len[t[i]] > lq) atomicOr(&A.flags[q[i]], 1u);
            }
        }
        census_count(q, wq, A.intervals, lane);
        if (!A.symmetric) {
            int ts[R], te[R];
            census_load<kVec>(A.ts, first, A.n_rec, -1, ts);
            census_load<kVec>(A.te, first, A.n_rec, -1, te);
#pragma unroll
            for (int i = 0; i < R; ++i)
                if (both[i] && ts[i] == 0) {
                    const int lt = A.len[t[i]];
                    if (te[i] == lt && A.len[q[i]] > lt) atomicOr(&A.flags[t[i]], 2u);
                }
            census_count(t, wt, A.intervals, lane);
        }
    }
}

// flag words -> one byte per read, and the number of reads with a flag
__global__ __launch_bounds__(256) void census_pack_kernel(const unsigned *__restrict__ flags, int32_t n_reads, uint8_t *__restrict__ out, unsigned long long *__restrict__ n_flagged)
{
    const int stride = (int)(gridDim.x * blockDim.x);
    unsigned mine = 0;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += stride) {
        const unsigned f = flags[r];
        out[r] = (uint8_t)f;
        mine += f ? 1u : 0u;
    }
    const int total = wave_reduce_add((int)mine);          // (all lanes are back together here)
    if (((int)threadIdx.x & (kWave - 1)) == 0 && total) atomicAdd(n_flagged, (unsigned long long)total);
}

} // namespace raft
