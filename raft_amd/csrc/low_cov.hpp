// low_cov.hpp -- the low-coverage runs of every read of a finished pass (raft_hip_low_coverage):
//
//     window w of read r (cov_offset[r] <= w < cov_offset[r + 1]) is low when cov[w] <= low_cov; a run is a maximal sequence of
//     consecutive low windows j1..j2 of ONE read;  low_s = j1 * reso,  low_e = min((j2 + 1) * reso, len[r])
//
// The first query of a finished pass whose output is a variable-length list per read (CSR) and not a fixed-size table: count, prefix,
// fill.  The array is read where it lies, in the form the pass wrote, as cov_hist.hpp and read_stats.hpp do: int32, or byte /
// uint16 codes when low_cov lies below the code's limit (a code at the limit is then above low_cov whatever the listed value is: the
// exception list is not needed); otherwise it is decoded into int32 first (low_cov_lib.hip).
//
//   * low_mark_kernel<E> streams cov[] ONCE: a lane takes kLowLaneWindows<E> consecutive windows per group of loads (8 int32 in two
//     16-byte loads, 8 / 16 codes in one), kLowInFlight groups in flight, and turns each group into 8 / 16 bits of the bitmap `bad`,
//     stored as consecutive bytes (byte pairs) across the wave: B / 8 bytes, 1/32 of the int32 array.  Everything after this kernel
//     reads bitmaps.  Fixed tiles, one per workgroup: no grid cap, no grid stride.
//   * low_read_starts_kernel sets the bit of every read's first window in a second, zeroed bitmap `rs`.  Run structure is then bit
//     arithmetic on 64-bit words with one carry bit from each neighbour word (low_cov_bits.hpp).
//   * low_count_kernel: a workgroup per tile of kLowTileWords words, a word per thread; the tile's number of run starts.
//   * low_prefix_kernel: ONE workgroup scans the tiles' counts (1.2e5 of them at human scale: 120 turns of a 1024-wide scan) and
//     publishes the total.  Launch boundaries carry what crosses workgroups: no look-back, no spinning (DESIGN I.0, I.8).
//   * low_fill_kernel reads the same words, ranks every start and end bit by a popcount prefix inside the workgroup -- the k-th start
//     and the k-th end of the array are the same run's; a tile whose first window continues a run ranks its ends one lower -- finds
//     the bit's read by bisecting cov_offset and writes low_s / low_e / the run's read directly.
//   * low_runs_kernel, a thread per run: the read's low windows, low bases and class bits (atomics on the read's own words);
//     low_reads_kernel, a thread per read: low_offset by bisecting the runs' read ids, the uncovered bit, the flag byte, the totals.
#pragma once
#include "raft_types.hpp"
#include "wave.hpp"
#include "device_scan.hpp"
#include "low_cov_bits.hpp"

namespace raft {

constexpr int kLowThreads = 256;
constexpr int kLowInFlight = 4;            // groups of loads a lane has in flight: 128 B of int32, 64 B of codes
constexpr int kLowMarkGroups = kLowThreads * kLowInFlight;   // lane groups of one workgroup of low_mark_kernel
constexpr int kLowTileWords = 256;         // bitmap words of one workgroup of low_count_kernel / low_fill_kernel (a word per thread)
constexpr int kLowPrefixThreads = 1024;
static_assert(kLowTileWords == kLowThreads, "a word per thread");

template <class E> struct LowIn;
template <> struct LowIn<int32_t> { static constexpr int vecs = 2; };
template <> struct LowIn<uint16_t> { static constexpr int vecs = 1; };
template <> struct LowIn<uint8_t> { static constexpr int vecs = 1; };
// consecutive windows of one lane group: 8 (int32, uint16) or 16 (bytes)
template <class E> constexpr int kLowLaneWindows = LowIn<E>::vecs * 16 / (int)sizeof(E);

// control words of one call: [0] n_runs, [1] low windows, [2] low bases, [3] reads with a run, [4] with an interior run, [5] uncovered,
// [6] a rank outside [0, n_runs) (never, unless the two bitmaps changed between count and fill)
constexpr int kLowCtlWords = 8;

struct LowRuns { int32_t *s, *e, *read; };                         // [n_runs] each
struct LowReads { unsigned *windows, *bases, *flag_words; };       // [n_reads] each, zeroed before the launch

// src: n_bins values or codes, 16-byte aligned, readable up to the next multiple of 16 bytes.  bad: n_groups groups of
// kLowLaneWindows<E> bits, whole words; bits from n_bins on are 0.
template <class E>
__global__ __launch_bounds__(kLowThreads) void low_mark_kernel(const E *__restrict__ src, long long n_bins, unsigned low_cov, void *__restrict__ bad,
                                                               long long n_groups)
{
    constexpr int V = LowIn<E>::vecs, W = kLowLaneWindows<E>, F = kLowInFlight, P = 16 / (int)sizeof(E);
    const uint4 *in = reinterpret_cast<const uint4 *>(src);
    const long long g0 = (long long)blockIdx.x * kLowMarkGroups + threadIdx.x;      // group f of the lane: g0 + f * kLowThreads
    uint4 a[F][V];
#pragma unroll
    for (int f = 0; f < F; ++f)
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const long long first = (g0 + (long long)f * kLowThreads) * W + j * P;   // the vector's first window
            a[f][j] = first < n_bins ? in[first / P] : make_uint4(~0u, ~0u, ~0u, ~0u);
        }
#pragma unroll
    for (int f = 0; f < F; ++f) {
        const long long g = g0 + (long long)f * kLowThreads;
        unsigned m = 0;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const unsigned w[4] = {a[f][j].x, a[f][j].y, a[f][j].z, a[f][j].w};
#pragma unroll
            for (int d = 0; d < 4; ++d)
#pragma unroll
                for (int k = 0; k < 4 / (int)sizeof(E); ++k) {
                    const unsigned v = sizeof(E) == 4 ? w[d] : sizeof(E) == 2 ? (w[d] >> (16 * k)) & 65535u : (w[d] >> (8 * k)) & 255u;
                    m |= (v <= low_cov ? 1u : 0u) << ((j * 4 + d) * (4 / (int)sizeof(E)) + k);
                }
        }
        const long long left = n_bins - g * W;                  // windows of the group that exist
        if (left < W) m &= left <= 0 ? 0u : (1u << (int)left) - 1u;
        if (g < n_groups) {
            if (W == 8) reinterpret_cast<uint8_t *>(bad)[g] = (uint8_t)m;
            else reinterpret_cast<uint16_t *>(bad)[g] = (uint16_t)m;
        }
    }
}

// rs: zeroed; off = cov_offset [n_reads + 1]
__global__ __launch_bounds__(kLowThreads) void low_read_starts_kernel(const long long *__restrict__ off, int32_t n_reads, unsigned long long *__restrict__ rs)
{
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    const long long w = off[r];
    if (off[r + 1] > w) atomicOr(&rs[w >> 6], 1ull << (int)(w & 63));
}

// start bits, end bits and the open-at-the-left-edge bit of word w (all 0 behind the bitmap)
__device__ __forceinline__ void low_word(const unsigned long long *__restrict__ bad, const unsigned long long *__restrict__ rs, long long w,
                                         long long n_words, uint64_t &starts, uint64_t &ends, uint64_t &open)
{
    starts = ends = open = 0;
    if (w >= n_words) return;
    const uint64_t b = bad[w], r = rs[w];
    LowEdges e;
    e.bad_prev63 = w > 0 ? bad[w - 1] >> 63 : 0;
    e.bad_next0 = w + 1 < n_words ? bad[w + 1] & 1ull : 0;
    e.rs_next0 = w + 1 < n_words ? rs[w + 1] & 1ull : 0;
    starts = low_starts(b, r, e); ends = low_ends(b, r, e); open = low_open_at_edge(b, r, e);
}

__global__ __launch_bounds__(kLowThreads) void low_count_kernel(const unsigned long long *__restrict__ bad, const unsigned long long *__restrict__ rs,
                                                                long long n_words, int32_t *__restrict__ tile_cnt)
{
    __shared__ int part[kLowThreads / kWave];
    uint64_t st, en, op;
    low_word(bad, rs, (long long)blockIdx.x * kLowTileWords + threadIdx.x, n_words, st, en, op);
    const int s = wave_reduce_add(__popcll(st));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
#pragma unroll
        for (int w = 0; w < kLowThreads / kWave; ++w) t += part[w];
        tile_cnt[blockIdx.x] = t;
    }
}

// one workgroup: tile_base[i] = runs that start in the tiles before tile i, ctl[0] = runs in all
__global__ __launch_bounds__(kLowPrefixThreads) void low_prefix_kernel(const int32_t *__restrict__ tile_cnt, long long n_tiles, long long *__restrict__ tile_base,
                                                                       unsigned long long *__restrict__ ctl)
{
    __shared__ long long lds[kLowPrefixThreads / 64 + 1];
    long long carry = 0;
    for (long long i0 = 0; i0 < n_tiles; i0 += kLowPrefixThreads) {
        const long long i = i0 + threadIdx.x;
        const long long v = i < n_tiles ? (long long)tile_cnt[i] : 0;
        long long tot;
        const long long ex = block_excl_scan64<kLowPrefixThreads>(v, &tot, lds);
        if (i < n_tiles) tile_base[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) ctl[0] = (unsigned long long)carry;
}

// the largest r in [0, n_reads) with off[r] <= w, for 0 <= w < off[n_reads]: the read that holds window w
__device__ __forceinline__ int low_read_of(const long long *__restrict__ off, int32_t n_reads, long long w)
{
    int lo = 0, hi = n_reads;                                   // off[lo] <= w < off[hi]
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= w) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kLowThreads) void low_fill_kernel(const unsigned long long *__restrict__ bad, const unsigned long long *__restrict__ rs,
                                                               long long n_words, const long long *__restrict__ tile_base,
                                                               const long long *__restrict__ off, const int32_t *__restrict__ len, int32_t n_reads,
                                                               int32_t reso, long long n_runs, LowRuns out, unsigned long long *__restrict__ ctl)
{
    __shared__ long long lds[kLowThreads / 64 + 1];
    __shared__ long long open_at_tile;
    const long long w = (long long)blockIdx.x * kLowTileWords + threadIdx.x;
    uint64_t st, en, op;
    low_word(bad, rs, w, n_words, st, en, op);
    if (threadIdx.x == 0) open_at_tile = (long long)op;
    long long tot;
    // (start and end counts of a word are at most 32 each and a tile's at most 2^13: the two scans share one 64-bit scan)
    const long long ex = block_excl_scan64<kLowThreads>((long long)__popcll(st) | ((long long)__popcll(en) << 32), &tot, lds);   // (its barriers publish open_at_tile)
    const long long base = tile_base[blockIdx.x];
    long long ks = base + (ex & 0xffffffffll);
    long long ke = base - open_at_tile + (ex >> 32);
    bool bad_rank = false;
    while (st) {
        const int b = __ffsll((unsigned long long)st) - 1;
        st &= st - 1;
        const long long win = w * kLowWordWindows + b;
        const int r = low_read_of(off, n_reads, win);
        if (ks >= 0 && ks < n_runs) { out.read[ks] = r; out.s[ks] = (int32_t)((win - off[r]) * reso); }
        else bad_rank = true;
        ++ks;
    }
    while (en) {
        const int b = __ffsll((unsigned long long)en) - 1;
        en &= en - 1;
        const long long win = w * kLowWordWindows + b;
        const int r = low_read_of(off, n_reads, win);
        const long long e = (win - off[r] + 1) * (long long)reso, l = len[r];
        if (ke >= 0 && ke < n_runs) out.e[ke] = (int32_t)(e < l ? e : l);
        else bad_rank = true;
        ++ke;
    }
    if (bad_rank) atomicOr(&ctl[6], 1ull);
}

// a thread per run: what the run adds to its read
__global__ __launch_bounds__(kLowThreads) void low_runs_kernel(LowRuns runs, long long n_runs, const long long *__restrict__ off, int32_t n_reads, int32_t reso,
                                                               LowReads out, unsigned long long *__restrict__ ctl)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_runs) return;
    const int r = runs.read[k];
    if (r < 0 || r >= n_reads) { atomicOr(&ctl[6], 1ull); return; }      // (a slot low_fill_kernel did not write: never, see kLowCtlWords)
    const int32_t s = runs.s[k], e = runs.e[k];
    const long long j1 = s / reso, j2 = ((long long)e + reso - 1) / reso - 1;      // (window j2 exists: j2 * reso < len, so the clamp keeps its index)
    atomicAdd(&out.windows[r], (unsigned)(j2 - j1 + 1));
    atomicAdd(&out.bases[r], (unsigned)(e - s));
    atomicOr(&out.flag_words[r], low_run_class(j1, j2, off[r + 1] - off[r]));
}

// a thread per entry of low_offset (n_reads + 1): the first run whose read is >= r; per read the uncovered bit, the flag byte, the totals
__global__ __launch_bounds__(kLowThreads) void low_reads_kernel(const int32_t *__restrict__ run_read, long long n_runs, const int32_t *__restrict__ len,
                                                                int32_t n_reads, int32_t uncovered_permille, LowReads acc,
                                                                long long *__restrict__ low_offset, uint8_t *__restrict__ low_flags,
                                                                unsigned long long *__restrict__ ctl)
{
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    long long windows = 0, bases = 0, counts = 0;
    if (r <= n_reads) {
        long long lo = 0, hi = n_runs;                          // run_read[< lo] < r <= run_read[>= hi]
        while (lo < hi) {
            const long long mid = lo + ((hi - lo) >> 1);
            if (run_read[mid] < r) lo = mid + 1; else hi = mid;
        }
        low_offset[r] = lo;
    }
    if (r < n_reads) {
        windows = acc.windows[r]; bases = acc.bases[r];
        unsigned f = acc.flag_words[r];
        if (low_uncovered(bases, len[r], uncovered_permille)) f |= kLowUncovered;
        low_flags[r] = (uint8_t)f;
        // (three counts of at most 64 per wave in one word)
        counts = (windows > 0 ? 1ll : 0ll) | ((f & kLowInterior) ? 1ll << 20 : 0ll) | ((f & kLowUncovered) ? 1ll << 40 : 0ll);
    }
    windows = wave_reduce_add64(windows); bases = wave_reduce_add64(bases); counts = wave_reduce_add64(counts);
    if ((threadIdx.x & 63) == 0 && counts + windows != 0) {
        atomicAdd(&ctl[1], (unsigned long long)windows);
        atomicAdd(&ctl[2], (unsigned long long)bases);
        if (counts & 0xfffff) atomicAdd(&ctl[3], (unsigned long long)(counts & 0xfffff));
        if ((counts >> 20) & 0xfffff) atomicAdd(&ctl[4], (unsigned long long)((counts >> 20) & 0xfffff));
        if (counts >> 40) atomicAdd(&ctl[5], (unsigned long long)(counts >> 40));
    }
}

} // namespace raft
