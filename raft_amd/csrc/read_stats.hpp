// read_stats.hpp -- the coverage summary of every read of a finished pass (raft_hip_read_stats):
//
//     cov_sum[r] = sum of cov[w],   cov_max[r] = max of cov[w] (0 without windows),   high_windows[r] = windows with cov[w] >= threshold
//                  over cov_offset[r] <= w < cov_offset[r + 1]
//
// A segmented reduction over the concatenated array by cov_offset.  The array is read where it lies, in the form the pass wrote, as
// cov_hist.hpp does: int32, or byte / uint16 codes (a code at the limit counts as the limit here; read_stats_exc_kernel then adds what
// the listed windows hold beyond it); a delta4 pass is decoded into int32 first (materialise_cov).
//
// Segments run from no window at all through one window to tens of thousands, so neither a lane nor a workgroup per read would do.
//   * spans: the array is dealt out in fixed spans of kReadStatsSpanGroups lane groups, grid-stride, ONE WAVE per span (a workgroup is
//     one wave: the waves share nothing, and a barrier is a wave barrier).  A lane group is kReadStatsLaneWindows<E> consecutive
//     windows (two 16-byte loads of int32, one of codes); group f of lane l lies at (f * 64 + l) groups into the span, so that a
//     load instruction of the wave covers consecutive memory, and a lane has kReadStatsInFlight groups of loads in flight;
//   * the span's first read is found once, by a 64-way search of cov_offset (every lane probes one position, a ballot narrows the
//     range: four dependent loads at 3.3e6 reads where a bisection takes 22);
//   * the ends of the kReadStatsSlots reads from there on go into a table in LDS, relative to the span; a lane finds its group's read
//     by bisecting the table (six LDS reads) and walks on from there.  A span that holds more reads than the table has slots (runs
//     of one-window reads) takes one more turn of the loop per table: the windows stay in registers;
//   * a group that lies in one read -- almost all -- is summed without a look at the table; a lane whose group crosses a boundary
//     hands the runs it closes to the slot's accumulator in LDS;
//   * the lanes' last runs are reduced by read across the wave (a segmented scan in six DPP steps: reads ascend with the lane) and
//     the last lane of each read adds to the slot's accumulator; distinct reads, distinct addresses;
//   * after the table's turn lane k writes slot k: a read that lies wholly inside the span is stored plainly into the zeroed
//     outputs, any other gets one 64-bit add, one max and one 32-bit add.  A read without coverage writes nothing.
#pragma once
#include "raft_types.hpp"
#include "wave.hpp"

namespace raft {

constexpr int kReadStatsThreads = 64;        // one wave per workgroup
constexpr int kReadStatsInFlight = 4;        // groups of loads a lane has in flight: 128 B of int32, 64 B of codes
constexpr int kReadStatsSpanGroups = 256;    // lane groups of one span (= threads x groups in flight): 2048 windows of int32 / uint16, 4096 bytes
constexpr int kReadStatsSlots = 64;          // reads of one table (one per lane)
constexpr int kReadStatsMaxBlocks = 4096;    // sixteen waves on each of the 256 CUs
static_assert(kReadStatsSpanGroups == kReadStatsThreads * kReadStatsInFlight, "a span is what one wave holds in registers");
static_assert(kReadStatsSlots == kWave && kReadStatsThreads == kWave, "lane k loads and writes slot k");
constexpr int kReadStatsFar = 1 << 30;       // table entry of a read that ends far beyond the span, or does not exist

template <class E> struct ReadStatsIn;
template <> struct ReadStatsIn<int32_t> { static constexpr int vecs = 2; static constexpr unsigned limit = 0; };
template <> struct ReadStatsIn<uint8_t> { static constexpr int vecs = 1; static constexpr unsigned limit = 255u; };
template <> struct ReadStatsIn<uint16_t> { static constexpr int vecs = 1; static constexpr unsigned limit = 65535u; };
// consecutive windows of one lane group: 8 (int32, uint16) or 16 (bytes)
template <class E> constexpr int kReadStatsLaneWindows = ReadStatsIn<E>::vecs * 16 / (int)sizeof(E);

struct ReadStatsOut { unsigned long long *sum; int32_t *max; int32_t *high; };   // [n_reads] each, zeroed before the launch

inline unsigned read_stats_grid(long long n_bins, int lane_windows)
{
    const long long span = (long long)kReadStatsSpanGroups * lane_windows;
    const long long want = (n_bins + span - 1) / span;
    return (unsigned)(want < 1 ? 1 : (want > kReadStatsMaxBlocks ? kReadStatsMaxBlocks : want));
}

// the largest r in [0, n_reads) with off[r] <= w, for 0 <= w < off[n_reads]; the same in every lane
__device__ __forceinline__ int read_stats_first_read(const long long *__restrict__ off, int32_t n_reads, long long w, int lane)
{
    int lo = 0, hi = n_reads;                                   // off[lo] <= w < off[hi]
    while (hi - lo > 1) {
        const int n = hi - lo, step = (n + kWave - 1) / kWave;
        const long long at = (long long)lo + (long long)(lane + 1) * step;
        const int p = at < hi ? (int)at : hi;
        const bool le = p < hi && off[p] <= w;
        const int cnt = __popcll(__ballot(le));                 // (the probes ascend with the lane: a prefix of the lanes says yes)
        const int nlo = lo + cnt * step;                        // cnt > 0: the last yes, below hi
        const long long nh = (long long)lo + (long long)(cnt + 1) * step;
        hi = uni(cnt == kWave ? hi : (nh < hi ? (int)nh : hi));
        lo = uni(nlo);
    }
    return lo;
}

// window i of a lane group held in V vectors
template <class E, class Fn>
__device__ __forceinline__ void read_stats_each(const uint4 *q, Fn fn)
{
    constexpr int P = 4 / (int)sizeof(E);
#pragma unroll
    for (int j = 0; j < ReadStatsIn<E>::vecs; ++j) {
        const unsigned w[4] = {q[j].x, q[j].y, q[j].z, q[j].w};
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
            for (int k = 0; k < P; ++k) {
                const unsigned v = sizeof(E) == 4 ? w[d] : sizeof(E) == 2 ? (w[d] >> (16 * k)) & 65535u : (w[d] >> (8 * k)) & 255u;
                fn((j * 4 + d) * P + k, v);
            }
    }
}

// entries of the table that are <= pos (fewer than kReadStatsSlots: the caller's pos lies below the last entry)
__device__ __forceinline__ int read_stats_slot(const int *tab, int pos)
{
    int k = 0;
#pragma unroll
    for (int st = kReadStatsSlots / 2; st >= 1; st >>= 1)
        if (tab[k + st - 1] <= pos) k += st;
    return k;
}

// One step of the segmented scan: a lane takes the partial result `ctrl` points it to when that lane holds the same key.
#define RAFT_RS_STEP(ctrl, rows)                                                                                       \
    {                                                                                                                  \
        const int ko = __builtin_amdgcn_update_dpp(-2, key, ctrl, rows, 0xf, false);                                   \
        const unsigned lo_ = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)s, ctrl, rows, 0xf, false);       \
        const unsigned hi_ = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(s >> 32), ctrl, rows, 0xf, false); \
        const int mo = __builtin_amdgcn_update_dpp(0, (int)m, ctrl, rows, 0xf, false);                                 \
        const unsigned co = (unsigned)__builtin_amdgcn_update_dpp(0, (int)c, ctrl, rows, 0xf, false);                  \
        if (ko == key) { s += ((unsigned long long)hi_ << 32) | lo_; m = (unsigned)mo > m ? (unsigned)mo : m; c += co; } \
    }

// (key, s, m, c) of every lane -> the same over the lanes up to and including it that hold its key; keys ascend with the lane (equal
// keys are neighbours), -2 is nobody's key.  EXEC must be all ones.
__device__ __forceinline__ void read_stats_seg_scan(int key, unsigned long long &s, unsigned &m, unsigned &c)
{
    RAFT_RS_STEP(0x111, 0xf) // row_shr:1
    RAFT_RS_STEP(0x112, 0xf) // row_shr:2
    RAFT_RS_STEP(0x114, 0xf) // row_shr:4
    RAFT_RS_STEP(0x118, 0xf) // row_shr:8
    RAFT_RS_STEP(0x142, 0xa) // row_bcast:15 into rows 1,3
    RAFT_RS_STEP(0x143, 0xc) // row_bcast:31 into rows 2,3
}
#undef RAFT_RS_STEP

// src: n_bins values or codes, 16-byte aligned, readable up to the next multiple of 16 bytes; off = cov_offset [n_reads + 1]
template <class E>
__global__ __launch_bounds__(kReadStatsThreads) void read_stats_kernel(const E *__restrict__ src, long long n_bins, const long long *__restrict__ off,
                                                                       int32_t n_reads, unsigned thr, ReadStatsOut out)
{
    constexpr int V = ReadStatsIn<E>::vecs, W = kReadStatsLaneWindows<E>, F = kReadStatsInFlight, T = kReadStatsSlots;
    constexpr int S = kReadStatsSpanGroups * W;
    __shared__ int tab[T];
    __shared__ unsigned long long acc_s[T];
    __shared__ unsigned acc_m[T], acc_c[T];
    const int lane = (int)threadIdx.x;
    const long long n_spans = (n_bins + S - 1) / S;
    const uint4 *in = reinterpret_cast<const uint4 *>(src);
    for (long long sp = blockIdx.x; sp < n_spans; sp += gridDim.x) {
        const long long w0 = sp * S;
        const int n_span = (int)(n_bins - w0 < (long long)S ? n_bins - w0 : (long long)S);
        uint4 a[F][V];
#pragma unroll
        for (int f = 0; f < F; ++f)
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const int first = (f * kWave + lane) * W + j * (16 / (int)sizeof(E));     // the vector's first window, in the span
                a[f][j] = first < n_span ? in[(w0 + first) / (16 / (int)sizeof(E))] : make_uint4(0u, 0u, 0u, 0u);
            }
        int r_base = read_stats_first_read(off, n_reads, w0, lane);
        long long start0 = off[r_base] - w0;          // where slot 0's read begins (<= 0 in the first turn)
        int lo_rel = 0;                               // the turn takes the windows [lo_rel, hi_rel) of the span
        for (;;) {
            const long long idx = (long long)r_base + 1 + lane;
            long long e = idx <= (long long)n_reads ? off[idx] - w0 : (long long)kReadStatsFar;
            if (e > (long long)kReadStatsFar) e = kReadStatsFar;
            __syncthreads();                          // (the turn before is through with the table)
            tab[lane] = (int)e; acc_s[lane] = 0ull; acc_m[lane] = 0u; acc_c[lane] = 0u;
            __syncthreads();
            const int last = tab[T - 1];
            const int hi_rel = last < n_span ? last : n_span;
#pragma unroll
            for (int f = 0; f < F; ++f) {
                // (the group's vectors as this turn's own values: the compiler otherwise unpacks and compares every window of the
                // span ahead of the loop over the turns, and holds 180 to 256 registers)
                uint4 q[V];
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    q[j] = a[f][j];
                    asm volatile("" : "+v"(q[j].x), "+v"(q[j].y), "+v"(q[j].z), "+v"(q[j].w));
                }
                const int g0 = (f * kWave + lane) * W;
                int key;
                unsigned long long s = 0ull;
                unsigned m = 0u, c = 0u;
                if (g0 + W <= lo_rel) key = -1;
                else if (g0 >= hi_rel) key = T;
                else {
                    int k = read_stats_slot(tab, g0 > lo_rel ? g0 : lo_rel);
                    int end = tab[k];
                    if (g0 >= lo_rel && g0 + W <= hi_rel && g0 + W <= end) {
                        read_stats_each<E>(q, [&](int, unsigned v) { s += v; m = v > m ? v : m; c += v >= thr ? 1u : 0u; });
                    } else {
                        read_stats_each<E>(q, [&](int i, unsigned v) {
                            const int pos = g0 + i;
                            if (pos >= lo_rel && pos < hi_rel) {
                                while (pos >= end) {      // the run of slot k is closed (k stays below T: pos < hi_rel <= tab[T - 1])
                                    if (s) { atomicAdd(&acc_s[k], s); atomicMax(&acc_m[k], m); atomicAdd(&acc_c[k], c); }
                                    s = 0ull; m = 0u; c = 0u;
                                    ++k; end = tab[k];
                                }
                                s += v; m = v > m ? v : m; c += v >= thr ? 1u : 0u;
                            }
                        });
                    }
                    key = k;
                }
                read_stats_seg_scan(key, s, m, c);
                const int next_key = __shfl_down(key, 1, kWave);
                if ((lane == kWave - 1 || next_key != key) && key >= 0 && key < T && s) {
                    atomicAdd(&acc_s[key], s); atomicMax(&acc_m[key], m); atomicAdd(&acc_c[key], c);
                }
            }
            __syncthreads();
            {
                const unsigned long long s = acc_s[lane];
                if (s) {                                  // (threshold >= 1: a read whose sum is 0 has max 0 and no high window)
                    const long long r = (long long)r_base + lane;
                    const long long begin = lane == 0 ? start0 : (long long)tab[lane - 1];
                    const unsigned m = acc_m[lane], c = acc_c[lane];
                    if (begin >= 0 && tab[lane] <= n_span) {           // wholly inside the span: nobody else writes this read
                        out.sum[r] = s; out.max[r] = (int32_t)m; out.high[r] = (int32_t)c;
                    } else {
                        atomicAdd(&out.sum[r], s); atomicMax(&out.max[r], (int32_t)m);
                        if (c) atomicAdd(&out.high[r], (int32_t)c);
                    }
                }
            }
            if (last >= n_span) break;
            lo_rel = last; start0 = last; r_base += T;
        }
    }
}

// The windows a width-1 / width-2 pass listed (value >= the code's limit), in no particular order: the main kernel has counted each
// as the limit.  A lane per entry: its read by bisection of cov_offset, value - limit onto the sum, the maximum raised, and one more
// high window only where the main kernel saw none (limit < threshold <= value).
__global__ __launch_bounds__(256) void read_stats_exc_kernel(const long long *__restrict__ idx, const int32_t *__restrict__ val, long long n,
                                                             const long long *__restrict__ off, int32_t n_reads, unsigned limit, unsigned thr,
                                                             ReadStatsOut out)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const long long w = idx[i];
        const unsigned v = (unsigned)val[i];
        int lo = 0, hi = n_reads;                                   // off[lo] <= w < off[hi]
        while (hi - lo > 1) {
            const int mid = lo + ((hi - lo) >> 1);
            if (off[mid] <= w) lo = mid; else hi = mid;
        }
        if (v > limit) atomicAdd(&out.sum[lo], (unsigned long long)(v - limit));
        atomicMax(&out.max[lo], (int32_t)v);
        if (limit < thr && thr <= v) atomicAdd(&out.high[lo], 1);
    }
}

} // namespace raft
