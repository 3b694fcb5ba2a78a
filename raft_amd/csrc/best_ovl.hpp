// best_ovl.hpp -- the best overlap of every read end (raft_hip_best_overlaps_device / _host, include/raft_hip_best.h): per read and
// end the greatest key of best_ovl_rule.hpp among the dovetail views whose two reads are not left out, whether the choice is mutual,
// the totals.
//
// Three kernels, none of which waits for another workgroup:
//   * best_digest_kernel: len | (skip != 0) << 31 per read in one 32-bit word, so that the stream gathers one word per id and not a
//     length and a byte.  (A length below 0 becomes 0: no record on such a read is valid, as under ends_kind.)
//   * best_kernel<kVec>, a streaming kernel of record_stream.hpp's shape that reads the stream exactly as ends_kernel does: the
//     six columns and the lane's four strand bytes (25 B per record in).  It evaluates ends_kind and reduces the candidates' keys
//     into a uint64 [2 * n_reads] table, cleared before every launch.
//       - query side: the column is mostly sorted runs, so equal neighbouring ids are joined before anything leaves the wave:
//         join_runs over the pair (5' key, 3' key) with max as the combine.  What leaves is at most one 64-bit atomicMax per run,
//         wave and end, and only for a key that is not 0.
//       - target side: the column is random and only a dovetail between two reads that are not left out has a key, so nothing is
//         joined: each key goes to its slot directly, behind a relaxed load of the slot that skips a key which cannot win (the
//         table only grows within a launch, so a stale value is a smaller one and skips less, never wrongly).
//       - an id outside [0, n_reads) in either column: the first bad record is kept, the record has no view.
//       - candidates and left_out are kept per lane and leave with one atomic per wave (lane 0 the first, lane 1 the second).
//   * best_pairs_kernel: one lane per read handles both of its slots -- it unpacks them, reads the two partner slots for mutuality,
//     writes partner and span (one 8-byte store each) and the flag byte (one plain store: no two lanes share a byte); the read
//     totals are kept per lane and leave with one atomic per wave.
#pragma once
#include "record_stream.hpp"
#include "best_ovl_rule.hpp"

namespace raft {

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

__global__ __launch_bounds__(256) void best_digest_kernel(const int32_t *__restrict__ len, const uint8_t *__restrict__ skip, int32_t n_reads,
                                                          unsigned *__restrict__ dig)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += stride) {
        const int32_t l = len[r];
        dig[r] = (l < 0 ? 0u : (unsigned)l) | ((skip && skip[r]) ? kBestSkipBit : 0u);
    }
}

// the value of best_kernel's join: the greatest 5' and 3' key of a run (0: no candidate); two shuffles
struct BestKeys { unsigned long long k5, k3; };

__device__ __forceinline__ BestKeys join_shfl_up(BestKeys v, int d) { return BestKeys{join_shfl_up(v.k5, d), join_shfl_up(v.k3, d)}; }

template <bool kVec>
__global__ __launch_bounds__(kStreamThreads) void best_kernel(BestArgs A)
{
    constexpr int R = kStreamLaneRecords;
    const int lane = (int)threadIdx.x & (kWave - 1);
    const unsigned n_reads = (unsigned)A.n_reads;
    const unsigned views = A.symmetric ? 1u : 2u;
    unsigned tot[2] = {0, 0};                              // candidates, left_out
    stream_for_each_group(A.n_rec, lane, [&](const long long first) {
        LaneRecords r;
        stream_load_records<kVec>(A.qid, A.qs, A.qe, A.tid, A.ts, A.te, first, A.n_rec, true, r);
        const unsigned rev4 = stream_load_bytes<kVec>(A.strand, first, A.n_rec);
        BestKeys key[R];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const IdsValid v = stream_check_ids(first + i < A.n_rec, first + i, r.q[i], r.t[i], n_reads, A.ctl);
            const bool rev = ((rev4 >> (8 * i)) & 0xFFu) != 0;
            key[i] = BestKeys{0, 0};
            if (v.q && v.t) {
                const unsigned dq = A.dig[r.q[i]], dt = A.dig[r.t[i]];
                const int kind = ends_kind(r.q[i], r.qs[i], r.qe[i], (int32_t)(dq & ~kBestSkipBit), r.t[i], r.ts[i], r.te[i],
                                           (int32_t)(dt & ~kBestSkipBit), rev, A.max_overhang, A.min_ratio);
                const int eq = best_end_of(kind);
                if (eq >= 0) {
                    if ((dq | dt) & kBestSkipBit) tot[1] += views;
                    else {
                        tot[0] += views;
                        const int32_t span = r.qe[i] - r.qs[i] < r.te[i] - r.ts[i] ? r.qe[i] - r.qs[i] : r.te[i] - r.ts[i];
                        const unsigned long long kq = best_pack(span, r.t[i], rev);
                        if (eq == 0) key[i].k5 = kq; else key[i].k3 = kq;
                        if (!A.symmetric) {
                            const unsigned long long kt = best_pack(span, r.q[i], rev);
                            unsigned long long *slot = &A.tab[2 * (size_t)(unsigned)r.t[i] + (unsigned)best_end_of(ends_target_view(kind, rev))];
                            if (__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < kt) atomicMax(slot, kt);
                        }
                    }
                }
            }
        }
        // tab[2 * id + E] = max(itself, the greatest key of end E among the wave's records with that id); a key of 0 goes nowhere
        join_runs(r.q, key, lane,
                  [](BestKeys a, BestKeys b) { return BestKeys{a.k5 > b.k5 ? a.k5 : b.k5, a.k3 > b.k3 ? a.k3 : b.k3}; },
                  [&](int id, BestKeys m) {
                      if (m.k5) atomicMax(&A.tab[2 * (size_t)(unsigned)id], m.k5);
                      if (m.k3) atomicMax(&A.tab[2 * (size_t)(unsigned)id + 1], m.k3);
                  });
    });
    // (all lanes of the wave are back together here)
    wave_flush_totals(tot, &A.ctl[kBestCtlViews], lane);
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
    wave_flush_totals(tot, &ctl[kBestCtlReads], lane);      // (all lanes are back together here)
}

} // namespace raft
