// ovl_class.hpp -- the record stream against the repeat annotation (raft_hip_repeat_overlaps_device / _host, include/raft_hip_ovl.h):
// one class byte per record (which side lies in the repeats of its read, which touches them, who is contained) and, per read, the
// sides that touch / lie in a repeat and whether everything that contains the read does so inside a repeat of the container.
//
// Two kernels and a small one behind them:
//   ovl_digest_kernel   a lane per read: checks the read's slice of rep_offset and sweeps its runs in ascending rep_s with a running
//                       covered-to position, which gives the pieces of the set union U(r).  8 bytes per read come out (OvlDigest):
//                           x <= y   U(r) is the one piece [x, y) -- or empty, {0, 0}: a read without a run, or with empty runs only
//                           x >  y   several pieces inside the hull [y, x): the side goes to the CSR arrays
//                       so a side on a read without repeats (two reads in three of a human set) is class 0 after one 8-byte gather,
//                       a read whose runs are one piece (one run, or runs joined by their flanks) needs nothing else either, and the
//                       rest is sent on only when the side reaches into the hull.
//   ovl_class_kernel    a streaming kernel of record_stream.hpp's shape (24 B in and 1 B out per record: the four class bytes of a lane
//                       leave as one 32-bit store) with the lookup of both sides in it, the length gather for the qs == 0 / ts == 0
//                       candidates only, and join_runs for the per-read tallies with the flags as packed weight (ovl_count).
//   ovl_reads_kernel    flag words -> one byte per read, tally words -> the two counts, the two totals over the reads.
// The record kernel reads ctl[kOvlBadOffsets] first and leaves when the digest kernel found rep_offset broken: it would read out of bounds.
#pragma once
#include "raft_types.hpp"
#include "wave.hpp"
#include "record_stream.hpp"

namespace raft {

// control words (unsigned long long each)
constexpr int kOvlFirstBad = 0;          // smallest record index with an id out of range; ~0 = none
constexpr int kOvlBadOffsets = 1;        // != 0: rep_offset is not what the header asks for
constexpr int kOvlRecTotals = 2;         // q_touch, t_touch, q_repeat, t_repeat, both_repeat, q_contained, t_contained
constexpr int kOvlReadTotals = 9;        // reads contained, reads repeat-contained
constexpr int kOvlCtlWords = 11;

struct OvlDigest { int32_t x, y; };

struct OvlArgs {
    const int32_t *len, *qid, *qs, *qe, *tid, *ts, *te;      // ts / te may be NULL (the target bits are then 0)
    long long n_rec;
    int32_t n_reads, symmetric, min_anchor;
    const long long *rep_off;
    const int32_t *rep_s, *rep_e;
    const OvlDigest *digest;
    uint8_t *cls;                                            // [n_rec], 4-byte aligned
    unsigned long long *tally;                               // [n_reads], zeroed before the launch: sides with TOUCH | sides with REPEAT << 32
    unsigned *flags;                                         // [n_reads], zeroed before the launch
    unsigned long long *ctl;
};

__global__ __launch_bounds__(256) void ovl_digest_kernel(const long long *__restrict__ rep_off, const int32_t *__restrict__ rep_s,
                                                         const int32_t *__restrict__ rep_e, int32_t n_reads, long long n_rep,
                                                         OvlDigest *__restrict__ digest, unsigned long long *__restrict__ ctl)
{
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_reads) return;
    if (r == n_reads) {                                      // the one lane behind the reads: the two ends
        if (rep_off[0] != 0 || rep_off[n_reads] != n_rep) atomicOr(&ctl[kOvlBadOffsets], 1ull);
        return;
    }
    const long long k0 = rep_off[r], k1 = rep_off[r + 1];
    OvlDigest d{0, 0};
    if (k0 < 0 || k1 < k0 || k1 > n_rep) {
        atomicOr(&ctl[kOvlBadOffsets], 1ull);
    } else {
        int pieces = 0;
        int32_t lo = 0, hi = 0, first = 0;                   // the open piece [lo, hi); where the first piece began
        for (long long k = k0; k < k1; ++k) {
            const int32_t s = rep_s[k], e = rep_e[k];
            if (e <= s) continue;
            if (pieces == 0) { pieces = 1; lo = first = s; hi = e; }
            else if (s <= hi) hi = e > hi ? e : hi;          // (reaches the open piece: the same piece of the union)
            else { ++pieces; lo = s; hi = e; }
        }
        if (pieces == 1) d = OvlDigest{lo, hi};
        else if (pieces > 1) d = OvlDigest{hi, first};       // hull [first, hi), written the wrong way round
    }
    digest[r] = d;
}

// One side [a, b) on read r: bit 0 = REPEAT, bit 2 = TOUCH (the query side's bits; the target side's are these shifted by one).
__device__ __forceinline__ unsigned ovl_side(const OvlArgs &A, const OvlDigest d, int r, int a, int b)
{
    if (b <= a) return 0u;                                   // span 0: nothing of it lies anywhere
    long long rep = 0;
    if (d.x <= d.y) {
        const int lo = a > d.x ? a : d.x, hi = b < d.y ? b : d.y;
        if (hi <= lo) return 0u;
        rep = (long long)hi - lo;
    } else {
        if ((b < d.x ? b : d.x) <= (a > d.y ? a : d.y)) return 0u;       // outside the hull
        const long long k1 = A.rep_off[r + 1];
        int cur = a;                                         // covered up to here
        for (long long k = A.rep_off[r]; k < k1; ++k) {
            const int s = A.rep_s[k];
            if (s >= b) break;                               // (ascending starts: nothing behind reaches the side)
            const int e = A.rep_e[k];
            const int lo = s > cur ? s : cur, hi = e < b ? e : b;
            if (hi > lo) { rep += (long long)hi - lo; cur = hi; }
        }
        if (rep == 0) return 0u;
    }
    const long long unique = (long long)b - a - rep;
    return 4u | (unique < (long long)A.min_anchor ? 1u : 0u);
}

// join_runs for the two tallies of a read at once: w = TOUCH | REPEAT << 16 of each record, summed over equal neighbouring ids -- a
// wave has kStreamWaveRecords records, so neither half overflows into the other -- and one 64-bit add per run and wave, the halves
// 32 bits apart.  A target column is random ids: one atomic per side that touches a repeat instead of one per tally.
static_assert(kStreamWaveRecords < (1 << 16), "a wave's sides on one read fit a half of the packed weight");

__device__ __forceinline__ void ovl_count(const int (&id)[kStreamLaneRecords], const unsigned (&w)[kStreamLaneRecords], unsigned long long *__restrict__ cnt, int lane)
{
    join_runs(id, w, lane, JoinAdd{}, [cnt](int r, unsigned x) {
        if (x) atomicAdd(&cnt[r], (unsigned long long)(x & 0xFFFFu) | ((unsigned long long)(x >> 16) << 32));
    });
}

template <bool kVec>
__global__ __launch_bounds__(kStreamThreads) void ovl_class_kernel(OvlArgs A)
{
    constexpr int R = kStreamLaneRecords;
    if (A.ctl[kOvlBadOffsets]) return;                       // (uniform: the digest kernel's verdict, written before this launch)
    const int lane = (int)threadIdx.x & (kWave - 1);
    const unsigned n_reads = (unsigned)A.n_reads;
    const bool targets = A.ts != nullptr;
    unsigned tot[7] = {0, 0, 0, 0, 0, 0, 0};
    stream_for_each_group(A.n_rec, lane, [&](const long long first) {
        LaneRecords r;
        stream_load_records<kVec>(A.qid, A.qs, A.qe, A.tid, A.ts, A.te, first, A.n_rec, targets, r);
        // the gathers of the lane's eight sides first, all in flight together: what is done with them follows
        OvlDigest dq[R], dt[R];
        bool ok[R];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const IdsValid v = stream_check_ids(first + i < A.n_rec, first + i, r.q[i], r.t[i], n_reads, &A.ctl[kOvlFirstBad]);
            ok[i] = v.q && v.t;
            dq[i] = dt[i] = OvlDigest{0, 0};
            if (ok[i]) {
                dq[i] = A.digest[r.q[i]];
                if (targets) dt[i] = A.digest[r.t[i]];
            }
        }
        unsigned cls4 = 0, wq[R], wt[R];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const bool both = ok[i];
            unsigned c = 0;
            if (both) {
                c = ovl_side(A, dq[i], r.q[i], r.qs[i], r.qe[i]);
                if (targets) c |= ovl_side(A, dt[i], r.t[i], r.ts[i], r.te[i]) << 1;
                // containment looks at the start before it gathers any length
                if (r.qs[i] == 0) {
                    const int lq = A.len[r.q[i]];
                    if (r.qe[i] == lq && A.len[r.t[i]] > lq) {
                        c |= 16u;
                        ovl_flag(&A.flags[r.q[i]], (c & 2u) ? 1u : 3u);          // the container is the target side
                    }
                }
                if (targets && r.ts[i] == 0) {
                    const int lt = A.len[r.t[i]];
                    if (r.te[i] == lt && A.len[r.q[i]] > lt) {
                        c |= 32u;
                        if (!A.symmetric) ovl_flag(&A.flags[r.t[i]], (c & 1u) ? 1u : 3u);   // (a side the census does not count otherwise)
                    }
                }
            }
            cls4 |= c << (8 * i);
            wq[i] = ((c >> 2) & 1u) | (c & 1u) << 16;
            const bool t_counts = both && !A.symmetric && r.t[i] != r.q[i];
            wt[i] = t_counts ? ((c >> 3) & 1u) | ((c >> 1) & 1u) << 16 : 0u;
            tot[0] += (c >> 2) & 1u; tot[1] += (c >> 3) & 1u; tot[2] += c & 1u; tot[3] += (c >> 1) & 1u;
            tot[4] += (c & 3u) == 3u ? 1u : 0u; tot[5] += (c >> 4) & 1u; tot[6] += (c >> 5) & 1u;
        }
        if (A.cls) stream_store_bytes<true>(A.cls, first, A.n_rec, cls4);        // (cls is 4-byte aligned whatever the columns are)
        // the tallies: a wave none of whose sides has the flag adds nothing (the branches are the wave's: EXEC stays all ones inside)
        if (__any((int)(wq[0] | wq[1] | wq[2] | wq[3]))) ovl_count(r.q, wq, A.tally, lane);
        if (__any((int)(wt[0] | wt[1] | wt[2] | wt[3]))) ovl_count(r.t, wt, A.tally, lane);
    });
    // (all lanes are back together here)
    wave_flush_totals(tot, &A.ctl[kOvlRecTotals], lane);
}

// flag words -> one byte per read, the tally words -> the two counts; reads that are contained, and those contained only inside repeats
__global__ __launch_bounds__(256) void ovl_reads_kernel(const unsigned *__restrict__ flags, const unsigned long long *__restrict__ tally, int32_t n_reads,
                                                        uint8_t *__restrict__ out, int32_t *__restrict__ touch, int32_t *__restrict__ repeat,
                                                        unsigned long long *__restrict__ ctl)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    unsigned contained = 0, only_repeat = 0;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += stride) {
        const unsigned f = flags[r];
        out[r] = (uint8_t)f;
        const unsigned long long t = tally[r];
        touch[r] = (int32_t)(unsigned)t; repeat[r] = (int32_t)(unsigned)(t >> 32);
        contained += f & 1u;
        only_repeat += f == 1u ? 1u : 0u;
    }
    const int c = wave_reduce_add((int)contained), o = wave_reduce_add((int)only_repeat);
    if (((int)threadIdx.x & (kWave - 1)) == 0) {
        if (c) atomicAdd(&ctl[kOvlReadTotals], (unsigned long long)c);
        if (o) atomicAdd(&ctl[kOvlReadTotals + 1], (unsigned long long)o);
    }
}

} // namespace raft
