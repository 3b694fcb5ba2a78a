// census.hpp -- what a record stream says about each read (raft_hip_census_device / _host), independent of any pass:
//
//     intervals[r] = intervals the pass piles up on read r: one per record with qid == r and, unless symmetric, one per record with
//                    tid == r and tid != qid (chop.hpp:165-169 with repeat.hpp:48-58)
//     flags[r]     = bit 0: some record has qid == r, qs == 0, qe == len[r] and len[tid] > len[r]
//                    bit 1 (not symmetric only): some record has tid == r, ts == 0, te == len[r] and len[qid] > len[r]
//
// One streaming kernel of record_stream.hpp's shape (16 B per record in when symmetric, 24 otherwise):
//   * containment looks at qs == 0 (ts == 0) before it gathers any length: the two random reads of read_len happen for the few
//     candidates only, and the flag goes out with an atomic OR on the read's own word;
//   * counts: join_runs with the record's count as value, + and atomicAdd: one add goes out per run and wave.  The target column
//     takes the same route with weight 0 for a record on its query's own read.
//   * an id outside [0, n_reads) in either column: the first bad record is kept and nothing is counted for that side.
#pragma once
#include "raft_types.hpp"
#include "wave.hpp"
#include "record_stream.hpp"

namespace raft {

struct CensusArgs {
    const int32_t *len, *qid, *qs, *qe, *tid, *ts, *te;
    long long n_rec;
    int32_t n_reads, symmetric;
    unsigned *intervals, *flags;             // [n_reads] each, zeroed before the launch
    unsigned long long *err;                 // smallest record index with an id out of range; ~0 = none
};

// cnt[id] += the sum of w over the wave's records with that id; a record with w = 0 adds nothing whatever its id
__device__ __forceinline__ void census_count(const int (&id)[kStreamLaneRecords], const unsigned (&w)[kStreamLaneRecords], unsigned *__restrict__ cnt, int lane)
{
    join_runs(id, w, lane, JoinAdd{}, [cnt](int r, unsigned n) { if (n) atomicAdd(&cnt[r], n); });
}

template <bool kVec>
__global__ __launch_bounds__(kStreamThreads) void census_kernel(CensusArgs A)
{
    constexpr int R = kStreamLaneRecords;
    const int lane = (int)threadIdx.x & (kWave - 1);
    const unsigned n_reads = (unsigned)A.n_reads;
    // stream_for_each_group's loop and the four loads written out: under the helpers the compiler waits for the third column before it
    // asks for the fourth (it waits for two in this form), which costs the symmetric census 5 % of its time.  As there, the loop's
    // bound is the wave's, never the lane's: every lane of a wave takes part in join_runs' shuffles (EXEC all ones).
    const long long n_groups = (A.n_rec + R - 1) / R;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long g0 = (long long)blockIdx.x * blockDim.x + ((int)threadIdx.x & ~(kWave - 1)); g0 < n_groups; g0 += stride) {
        const long long first = (g0 + lane) * R;           // (at or beyond n_rec: a lane without records)
        int q[R], t[R], a[R], b[R];
        stream_load<kVec>(A.qid, first, A.n_rec, -1, q);
        stream_load<kVec>(A.tid, first, A.n_rec, -1, t);
        stream_load<kVec>(A.qs, first, A.n_rec, -1, a);
        stream_load<kVec>(A.qe, first, A.n_rec, -1, b);
        unsigned wq[R], wt[R];
        bool both[R];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const IdsValid v = stream_check_ids(first + i < A.n_rec, first + i, q[i], t[i], n_reads, A.err);
            wq[i] = v.q ? 1u : 0u;
            wt[i] = (!A.symmetric && v.t && t[i] != q[i]) ? 1u : 0u;
            both[i] = v.q && v.t;
            if (both[i] && a[i] == 0) {
                const int lq = A.len[q[i]];
                if (b[i] == lq && A.len[t[i]] > lq) atomicOr(&A.flags[q[i]], 1u);
            }
        }
        census_count(q, wq, A.intervals, lane);
        if (!A.symmetric) {
            int ts[R], te[R];
            stream_load<kVec>(A.ts, first, A.n_rec, -1, ts);
            stream_load<kVec>(A.te, first, A.n_rec, -1, te);
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
