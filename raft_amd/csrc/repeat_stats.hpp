// repeat_stats.hpp -- one row per repeat run (raft_hip_repeat_stats_device / _host, include/raft_hip_rst.h): the counted overlap sides
// that touch the run, span it end to end and lie inside it; the coverage of the finished pass over the run's windows; where the run
// sits in its read.
//
// Run ends do not ascend within a read (raft_hip_ovl.h), so no property selects a contiguous range of runs: the counts come from a
// walk over the read's runs, not from difference arrays.  Four kernels:
//   rst_digest_kernel   a lane per read plus one for the two ends of rep_offset: checks the read's slice and writes 16 bytes per read
//                       (RstDigest): where its runs begin, how many there are, and the hull [x, y) = [min s, max e) over the non-empty
//                       runs.  A side outside the hull touches nothing.  A read with exactly ONE non-empty run is written as that run
//                       alone (k0 = its index, n = 1: nothing counts the empty ones beside it), so its hull is the run and a side is
//                       answered from the gather.  It also writes the read of every run (run_read) for the two kernels over the runs.
//   rst_side_kernel     a streaming kernel of record_stream.hpp's shape, both digest gathers of a lane's records issued together.
//                       A side inside the hull of a read with several runs walks them in ascending rep_s, stops at the first
//                       s >= b, and sends its adds directly.  Sides on single-run reads -- the hot streaks of a sorted query column --
//                       go through join_runs with the three counts as packed weight (rst_count): equal neighbouring slots are joined
//                       within the lane and across the wave, and one pair of adds is sent per slot and wave.
//                       Counters are 16 bytes per run (RstSlot): touch and span share one 64-bit word, inside is the second.  All adds
//                       are positive, so the halves stay 32 bits apart and do not mix below 2^32 sides on a run.
//   rst_cov_kernel      a wave per run, grid-stride over the runs, the lanes striding over the run's windows of the int32 coverage:
//                       16-byte loads from the first window index that is a multiple of four, a scalar head before and a scalar tail
//                       behind.  One wave reduction of (sum in 64 bits, min, max, windows at or above the threshold) per run; no atomics.
//   rst_runs_kernel     a lane per run: unpacks the slot into the three int32 arrays, writes the flags byte, and reduces the summary's
//                       totals once per wave.
// The record kernel looks at ctl[kRstBadOffsets] first and leaves when the digest kernel found rep_offset broken: it would read out
// of bounds.  No kernel waits for another workgroup; every loop is bounded by a read's run count or a run's window count.
#pragma once
#include "raft_types.hpp"
#include "wave.hpp"
#include "record_stream.hpp"

namespace raft {

constexpr int kRstFieldBits = 10;                        // a count of the packed weight: touch | span << 10 | inside << 20
constexpr int kRstCovVec = 4;                            // windows of one 16-byte load
constexpr int kRstCovStep = kRstCovVec * kWave;          // windows one wave takes per step of the coverage kernel
constexpr int kRstCovThreads = 256;
constexpr int kRstCovMaxBlocks = 8192;
static_assert(kStreamWaveRecords < (1 << kRstFieldBits), "a wave's sides on one slot must fit one field of the packed weight");

// control words (unsigned long long each)
constexpr int kRstFirstBad = 0;          // smallest record index with an id out of range; ~0 = none
constexpr int kRstBadOffsets = 1;        // != 0: rep_offset is not what the header asks for
constexpr int kRstTotals = 2;            // empty, interior, touched, spanned, interior spanned, sides touch / span / inside, windows, cov_sum
constexpr int kRstNumTotals = 10;
constexpr int kRstCtlWords = kRstTotals + kRstNumTotals;

constexpr unsigned kRstEmpty = 1, kRstAtStart = 2, kRstAtEnd = 4;       // RAFT_HIP_RST_* (repeat_stats_lib.hip asserts it)

struct RstDigest { int32_t k0, n, x, y; };
// the counters of a run: ts = touch + (span << 32), c = inside; zeroed before the launch
struct RstSlot { unsigned long long ts, c; };

__global__ __launch_bounds__(256) void rst_digest_kernel(const long long *__restrict__ rep_off, const int32_t *__restrict__ rep_s,
                                                         const int32_t *__restrict__ rep_e, int32_t n_reads, long long n_rep,
                                                         RstDigest *__restrict__ digest, int32_t *__restrict__ run_read,
                                                         unsigned long long *__restrict__ ctl)
{
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_reads) return;
    if (r == n_reads) {                                      // the one lane behind the reads: the two ends
        if (rep_off[0] != 0 || rep_off[n_reads] != n_rep) atomicOr(&ctl[kRstBadOffsets], 1ull);
        return;
    }
    const long long k0 = rep_off[r], k1 = rep_off[r + 1];
    RstDigest d{0, 0, 0, 0};
    if (k0 < 0 || k1 < k0 || k1 > n_rep) {
        atomicOr(&ctl[kRstBadOffsets], 1ull);
    } else if (k1 > k0) {
        int real = 0;
        long long only = k0;                                 // the last non-empty run seen
        int32_t lo = 0, hi = 0;
        for (long long k = k0; k < k1; ++k) {
            run_read[k] = (int32_t)r;
            const int32_t s = rep_s[k], e = rep_e[k];
            if (e <= s) continue;
            lo = real ? (s < lo ? s : lo) : s;
            hi = real ? (e > hi ? e : hi) : e;
            ++real; only = k;
        }
        if (real == 1) d = RstDigest{(int32_t)only, 1, lo, hi};
        else if (real > 1) d = RstDigest{(int32_t)k0, (int32_t)(k1 - k0), lo, hi};
    }
    digest[r] = d;
}

struct RstArgs {
    const int32_t *qid, *qs, *qe, *tid, *ts, *te;            // ts / te may be NULL when symmetric
    long long n_rec;
    int32_t n_reads, symmetric;
    const int32_t *rep_s, *rep_e;
    const RstDigest *digest;
    RstSlot *slot;                                           // [n_rep], zeroed before the launch
    unsigned long long *ctl;
};

__device__ __forceinline__ void rst_add(RstSlot *__restrict__ slot, int id, unsigned x)
{
    constexpr unsigned kMask = (1u << kRstFieldBits) - 1u;
    atomicAdd(&slot[id].ts, (unsigned long long)(x & kMask) | ((unsigned long long)((x >> kRstFieldBits) & kMask) << 32));
    const unsigned inside = x >> (2 * kRstFieldBits);
    if (inside) atomicAdd(&slot[id].c, (unsigned long long)inside);
}

// join_runs for the three counts of a run at once: w = touch | span << 10 | inside << 20 of each record, summed over equal
// neighbouring slot ids -- a wave has kStreamWaveRecords records, so no field overflows into the next -- and one pair of adds per
// slot and wave.  A record with w = 0 adds nothing whatever its id: a side without a slot comes with id -1.
__device__ __forceinline__ void rst_count(const int (&id)[kStreamLaneRecords], const unsigned (&w)[kStreamLaneRecords], RstSlot *__restrict__ slot, int lane)
{
    join_runs(id, w, lane, JoinAdd{}, [slot](int k, unsigned x) { if (x) rst_add(slot, k, x); });
}

// One counted side [a, b) on the read with digest d.  A single-run read: the packed weight for the join comes back and *id is the
// run's slot.  Several runs: the walk, its adds sent from here; 0 comes back.
__device__ __forceinline__ unsigned rst_side(const RstArgs &A, const RstDigest d, int a, int b, int *id)
{
    *id = -1;
    if (b <= a || d.n == 0 || a >= d.y || b <= d.x) return 0u;          // (outside the hull: no run has e > a and s < b)
    if (d.n == 1) {                                          // the hull is the run: touched
        *id = d.k0;
        return 1u | (a <= d.x && b >= d.y ? 1u << kRstFieldBits : 0u) | (a >= d.x && b <= d.y ? 1u << (2 * kRstFieldBits) : 0u);
    }
    const int32_t *rs = A.rep_s + d.k0, *re = A.rep_e + d.k0;
    for (int k = 0; k < d.n; ++k) {
        const int s = rs[k];
        if (s >= b) break;                                   // (ascending starts: nothing behind reaches the side)
        const int e = re[k];
        if (e <= s || a >= e) continue;
        atomicAdd(&A.slot[d.k0 + k].ts, 1ull | (a <= s && b >= e ? 1ull << 32 : 0ull));
        if (a >= s && b <= e) atomicAdd(&A.slot[d.k0 + k].c, 1ull);
    }
    return 0u;
}

template <bool kVec>
__global__ __launch_bounds__(kStreamThreads) void rst_side_kernel(RstArgs A)
{
    constexpr int R = kStreamLaneRecords;
    if (A.ctl[kRstBadOffsets]) return;                       // (uniform: the digest kernel's verdict, written before this launch)
    const int lane = (int)threadIdx.x & (kWave - 1);
    const unsigned n_reads = (unsigned)A.n_reads;
    const bool targets = !A.symmetric;
    stream_for_each_group(A.n_rec, lane, [&](const long long first) {
        LaneRecords r;
        stream_load_records<kVec>(A.qid, A.qs, A.qe, A.tid, A.ts, A.te, first, A.n_rec, targets, r);
        // the gathers of the lane's eight sides first, all in flight together
        RstDigest dq[R], dt[R];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const IdsValid v = stream_check_ids(first + i < A.n_rec, first + i, r.q[i], r.t[i], n_reads, &A.ctl[kRstFirstBad]);
            dq[i] = dt[i] = RstDigest{0, 0, 0, 0};
            if (v.q && v.t) {
                dq[i] = A.digest[r.q[i]];
                if (targets && r.t[i] != r.q[i]) dt[i] = A.digest[r.t[i]];   // (a target side on its query's own read is not counted)
            }
        }
        int iq[R], it[R];
        unsigned wq[R], wt[R];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            wq[i] = rst_side(A, dq[i], r.qs[i], r.qe[i], &iq[i]);
            it[i] = -1; wt[i] = 0u;
            if (targets) wt[i] = rst_side(A, dt[i], r.ts[i], r.te[i], &it[i]);
        }
        // a wave none of whose sides is on a single-run read adds nothing (the branches are the wave's: EXEC stays all ones inside)
        if (__any((int)(wq[0] | wq[1] | wq[2] | wq[3]))) rst_count(iq, wq, A.slot, lane);
        if (__any((int)(wt[0] | wt[1] | wt[2] | wt[3]))) rst_count(it, wt, A.slot, lane);
    });
}

struct RstCovOut { int32_t *windows, *cov_min, *cov_max, *high; long long *cov_sum; };

struct RstCovAcc {
    long long sum; int mn, mx, high;
    __device__ __forceinline__ void take(int v, int thr)
    {
        sum += v; mn = v < mn ? v : mn; mx = v > mx ? v : mx; high += v >= thr ? 1 : 0;
    }
};

__global__ __launch_bounds__(kRstCovThreads) void rst_cov_kernel(const int32_t *__restrict__ cov, const long long *__restrict__ cov_off,
                                                                 const int32_t *__restrict__ rep_s, const int32_t *__restrict__ rep_e,
                                                                 const int32_t *__restrict__ run_read, long long n_rep, int32_t reso, int32_t threshold,
                                                                 const unsigned long long *__restrict__ ctl, RstCovOut out)
{
    if (ctl[kRstBadOffsets]) return;                         // (run_read is then not what it should be)
    const int lane = (int)threadIdx.x & (kWave - 1);
    const long long n_waves = (long long)gridDim.x * (kRstCovThreads / kWave);
    const int wave = uni((int)threadIdx.x >> 6);             // (the run, its bounds and the loops' ends stay scalar)
    for (long long k = (long long)blockIdx.x * (kRstCovThreads / kWave) + wave; k < n_rep; k += n_waves) {
        const long long s = rep_s[k], e = rep_e[k];
        const int r = run_read[k];
        const long long w0 = cov_off[r], W = cov_off[r + 1] - w0;
        long long j0 = (s > 0 ? s : 0) / reso, j1 = e > 0 ? (e + reso - 1) / reso : 0;
        j1 = j1 < W ? j1 : W;
        if (e <= s || j1 < j0) j1 = j0;
        const long long g0 = w0 + j0, g1 = w0 + j1;          // the run's windows in the coverage array
        const long long body0 = (g0 + kRstCovVec - 1) & ~(long long)(kRstCovVec - 1), body1 = g1 & ~(long long)(kRstCovVec - 1);
        RstCovAcc acc{0, 0x7fffffff, 0, 0};
        if (body0 >= body1) {                                // no whole group: every window on its own
            for (long long g = g0 + lane; g < g1; g += kWave) acc.take(cov[g], threshold);
        } else {
            if (g0 + lane < body0) acc.take(cov[g0 + lane], threshold);                  // the head: at most three windows
            for (long long g = body0 + (long long)lane * kRstCovVec; g < body1; g += kRstCovStep) {
                const int4 v = *reinterpret_cast<const int4 *>(cov + g);
                acc.take(v.x, threshold); acc.take(v.y, threshold); acc.take(v.z, threshold); acc.take(v.w, threshold);
            }
            if (body1 + lane < g1) acc.take(cov[body1 + lane], threshold);               // the tail: at most three
        }
        // (all lanes are back together here)
        const long long sum = wave_reduce_add64(acc.sum);
        const int high = wave_reduce_add(acc.high);
        const int mx = __builtin_amdgcn_readlane(wave_incl_scan_max(acc.mx, 0), kWave - 1);
        const int mn = -__builtin_amdgcn_readlane(wave_incl_scan_max(-acc.mn, 0), kWave - 1);
        if (lane == 0) {
            const bool any = g1 > g0;
            out.windows[k] = (int32_t)(g1 - g0);
            out.cov_sum[k] = any ? sum : 0;
            out.cov_min[k] = any ? mn : 0;
            out.cov_max[k] = any ? mx : 0;
            out.high[k] = any ? high : 0;
        }
    }
}

inline unsigned rst_cov_grid(long long n_rep)
{
    const long long per = kRstCovThreads / kWave;
    const long long want = (n_rep + per - 1) / per;
    return (unsigned)(want < 1 ? 1 : (want > kRstCovMaxBlocks ? kRstCovMaxBlocks : want));
}

struct RstRunsArgs {
    const RstSlot *slot;
    const int32_t *rep_s, *rep_e, *run_read, *len;
    long long n_rep;
    const int32_t *windows;                                  // NULL: no coverage part
    const long long *cov_sum;
    int32_t *touch, *span, *inside;
    uint8_t *flags;
    unsigned long long *ctl;
};

__global__ __launch_bounds__(256) void rst_runs_kernel(RstRunsArgs A)
{
    if (A.ctl[kRstBadOffsets]) return;
    const long long stride = (long long)gridDim.x * blockDim.x;
    long long tot[kRstNumTotals] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < A.n_rep; k += stride) {
        const RstSlot sl = A.slot[k];
        const unsigned touch = (unsigned)sl.ts, span = (unsigned)(sl.ts >> 32), inside = (unsigned)sl.c;
        const int s = A.rep_s[k], e = A.rep_e[k];
        const unsigned f = (e <= s ? kRstEmpty : 0u) | (s <= 0 ? kRstAtStart : 0u) | (e >= A.len[A.run_read[k]] ? kRstAtEnd : 0u);
        A.touch[k] = (int32_t)touch; A.span[k] = (int32_t)span; A.inside[k] = (int32_t)inside;
        A.flags[k] = (uint8_t)f;
        tot[0] += f & kRstEmpty; tot[1] += f == 0u ? 1 : 0; tot[2] += touch ? 1 : 0; tot[3] += span ? 1 : 0;
        tot[4] += (f == 0u && span) ? 1 : 0; tot[5] += touch; tot[6] += span; tot[7] += inside;
        if (A.windows) { tot[8] += A.windows[k]; tot[9] += A.cov_sum[k]; }
    }
    // (all lanes are back together here)
#pragma unroll
    for (int i = 0; i < kRstNumTotals; ++i) {
        const long long total = wave_reduce_add64(tot[i]);
        if (((int)threadIdx.x & (kWave - 1)) == 0 && total) atomicAdd(&A.ctl[kRstTotals + i], (unsigned long long)total);
    }
}

} // namespace raft
