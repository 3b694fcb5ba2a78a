// cov_hist.hpp -- histogram of the finished pass's window coverage (raft_hip_cov_histogram).
//
//     hist[v] = windows with coverage v, 0 <= v < kCovHistBins - 1;   hist[kCovHistBins - 1] = windows with coverage >= kCovHistBins - 1
//
// The estimated coverage (-e, algoParams::est_cov: high_cov = (int)(est_cov * cov_mul), repeat.hpp:89-90) is the one number the path
// cannot run without, and the reference leaves it to the user (README.md:26-30).  The pileup's own window coverage peaks at the
// sequencing depth; the peak of this histogram is what raft_hip_estimate_coverage reads it from.  The array the histogram is made of
// is the pass's largest (8 GB of int32 at human scale): it is read where it lies, in the form the pass wrote --
//     int32 cov[]                      (output width 4)
//     byte / uint16 codes              (width 1 / 2: a code below the limit IS the value; a code at the limit is skipped here and its
//                                       window counted from the exception list by cov_hist_exc_kernel)
// -- and a delta4 pass is decoded into int32 first (materialise_cov).
//
// The input is the worst case for a naive histogram: neighbouring windows are mostly equal (the step is 0 for most of them, within
// +-7 for 99.8 %) and almost all mass lies within +-sqrt(depth) of one value, so one LDS atomic per window would queue up on a handful
// of addresses.  Hence
//   * run aggregation: a lane walks kCovHistLaneWindows<E> CONSECUTIVE windows per step (8 int32 in two 16-byte loads, 16 bytes of
//     codes in one) and issues one LDS add per run of equal values, not one per window; runs are not joined across lanes or steps;
//   * one private sub-histogram per wave of the workgroup (4 x 4096 x 4 B = 64 KiB of the CU's 160: two workgroups per CU), so that
//     the four waves never meet on an address; lanes of one wave that hit the same bin are serialised by the LDS (distinct bins next
//     to each other fall on distinct banks);
//   * kCovHistInFlight independent groups of loads in flight per lane (this step's and those a grid stride further on each:
//     pack_cov_kernel's shape);
//   * flush: after the workgroup's last step the four copies are summed bin by bin, strided over the workgroup, and the non-zero
//     sums -- a few dozen of the 4096 on real data -- go to the global 64-bit histogram with one atomicAdd each.
// 32-bit LDS counters cannot overflow: the launch (cov_hist_grid) gives a workgroup fewer than 2^31 windows.
#pragma once
#include "raft_types.hpp"

namespace raft {

constexpr int kCovHistBins = 4096;          // = RAFT_HIP_COV_HIST_BINS
constexpr int kCovHistThreads = 256;        // four waves, one sub-histogram each
constexpr int kCovHistWaves = kCovHistThreads / 64;
constexpr int kCovHistMaxBlocks = 512;      // two workgroups (2 x 64 KiB of LDS) on each of the 256 CUs: every workgroup is resident, and flushes once
constexpr int kCovHistInFlight = 4;         // groups of loads a lane has in flight: 128 B of int32, 64 B of codes (two workgroups per CU leave 8 waves to hide HBM's latency)
constexpr unsigned kCovHistSkip = 0xFFFFFFFFu;

// E = int32_t: values; uint8_t / uint16_t: codes of the transfer encoding (pack.hpp), whose limit is listed elsewhere
template <class E> struct CovHistIn;
template <> struct CovHistIn<int32_t> { static constexpr int vecs = 2; static constexpr bool has_skip = false; static constexpr unsigned limit = 0; };
template <> struct CovHistIn<uint8_t> { static constexpr int vecs = 1; static constexpr bool has_skip = true; static constexpr unsigned limit = 255u; };
template <> struct CovHistIn<uint16_t> { static constexpr int vecs = 1; static constexpr bool has_skip = true; static constexpr unsigned limit = 65535u; };
// consecutive windows a lane walks per group of loads: 8 (int32, uint16) or 16 (bytes)
template <class E> constexpr int kCovHistLaneWindows = CovHistIn<E>::vecs * 16 / (int)sizeof(E);

// blocks of the launch over n_groups lane groups (capped, grid-stride).  A workgroup sees at most ceil(n_groups / (grid * 256)) * 256
// groups of <= 16 windows: with grid >= n_bins / 2^30 that stays below 2^31 (the cap alone would do up to 2^39 windows).
inline unsigned cov_hist_grid(long long n_groups, long long n_bins)
{
    const long long per_step = (long long)kCovHistInFlight * kCovHistThreads;                // (groups a workgroup takes per step)
    const long long want = (n_groups + per_step - 1) / per_step;
    long long grid = want < 1 ? 1 : (want > kCovHistMaxBlocks ? kCovHistMaxBlocks : want);
    const long long floor_blocks = (n_bins >> 30) + 1;
    if (grid < floor_blocks) grid = floor_blocks;
    return (unsigned)grid;
}

__device__ __forceinline__ unsigned cov_hist_bin(unsigned v) { return v < (unsigned)(kCovHistBins - 1) ? v : (unsigned)(kCovHistBins - 1); }

// one run of `n` windows with key `key` (a bin, or kCovHistSkip) into the wave's copy
template <bool kSkip>
__device__ __forceinline__ void cov_hist_add(unsigned *h, unsigned key, unsigned n)
{
    if (kSkip && key == kCovHistSkip) return;
    atomicAdd(&h[key], n);
}

template <class E>
__device__ __forceinline__ unsigned cov_hist_key(unsigned v)
{
    if (CovHistIn<E>::has_skip && v == CovHistIn<E>::limit) return kCovHistSkip;
    return cov_hist_bin(v);
}

// Walks the values of one 16-byte vector in window order, extending the run (cur, cnt) that the lane carries through its group.
template <class E>
__device__ __forceinline__ void cov_hist_walk(const uint4 q, unsigned *h, unsigned &cur, unsigned &cnt)
{
    constexpr bool S = CovHistIn<E>::has_skip;
    const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int d = 0; d < 4; ++d) {
#pragma unroll
        for (int k = 0; k < 4 / (int)sizeof(E); ++k) {
            const unsigned v = sizeof(E) == 4 ? w[d] : sizeof(E) == 2 ? (w[d] >> (16 * k)) & 65535u : (w[d] >> (8 * k)) & 255u;
            const unsigned key = cov_hist_key<E>(v);
            if (key == cur) ++cnt;
            else { cov_hist_add<S>(h, cur, cnt); cur = key; cnt = 1; }
        }
    }
}

template <class E>
__device__ __forceinline__ void cov_hist_group(const uint4 *q, unsigned *h)
{
    // (the run starts as the first window's key with no window counted yet: the walk then counts that window like any other)
    unsigned cur = cov_hist_key<E>(sizeof(E) == 4 ? q[0].x : sizeof(E) == 2 ? q[0].x & 65535u : q[0].x & 255u), cnt = 0;
#pragma unroll
    for (int j = 0; j < CovHistIn<E>::vecs; ++j) cov_hist_walk<E>(q[j], h, cur, cnt);
    cov_hist_add<CovHistIn<E>::has_skip>(h, cur, cnt);
}

__device__ __forceinline__ void cov_hist_clear(unsigned (*lds)[kCovHistBins])
{
    uint4 *z = reinterpret_cast<uint4 *>(&lds[0][0]);
    for (int i = (int)threadIdx.x; i < kCovHistWaves * kCovHistBins / 4; i += kCovHistThreads) z[i] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
}

// the workgroup's counts into the global histogram: all-zero bins -- most of the 4096 -- cost four LDS reads and nothing else
__device__ __forceinline__ void cov_hist_flush(unsigned (*lds)[kCovHistBins], unsigned long long *__restrict__ hist)
{
    __syncthreads();
    for (int b = (int)threadIdx.x; b < kCovHistBins; b += kCovHistThreads) {
        unsigned s = 0;
#pragma unroll
        for (int w = 0; w < kCovHistWaves; ++w) s += lds[w][b];       // (below 2^31 in total: cov_hist_grid)
        if (s) atomicAdd(&hist[b], (unsigned long long)s);
    }
}

// src: n_bins values or codes, 16-byte aligned.  Lane groups of kCovHistLaneWindows<E> windows are dealt out grid-stride; the
// windows behind the last whole group (fewer than one group's worth) are taken one by one by the first lanes of workgroup 0.
template <class E>
__global__ __launch_bounds__(kCovHistThreads) void cov_hist_kernel(const E *__restrict__ src, long long n_bins, unsigned long long *__restrict__ hist)
{
    __shared__ unsigned lds[kCovHistWaves][kCovHistBins];
    constexpr int V = CovHistIn<E>::vecs, W = kCovHistLaneWindows<E>;
    cov_hist_clear(lds);
    unsigned *h = lds[threadIdx.x >> 6];
    const long long n_groups = n_bins / W;
    const long long stride = (long long)gridDim.x * blockDim.x;
    long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const uint4 *in = reinterpret_cast<const uint4 *>(src);
    for (; g + (kCovHistInFlight - 1) * stride < n_groups; g += kCovHistInFlight * stride) {     // every group's loads issued before the first is walked
        uint4 a[kCovHistInFlight][V];
#pragma unroll
        for (int f = 0; f < kCovHistInFlight; ++f)
#pragma unroll
            for (int j = 0; j < V; ++j) a[f][j] = in[(g + f * stride) * V + j];
#pragma unroll
        for (int f = 0; f < kCovHistInFlight; ++f) cov_hist_group<E>(a[f], h);
    }
    for (; g < n_groups; g += stride) {                  // (at most kCovHistInFlight - 1 more)
        uint4 a[V];
#pragma unroll
        for (int j = 0; j < V; ++j) a[j] = in[g * V + j];
        cov_hist_group<E>(a, h);
    }
    if (blockIdx.x == 0 && (long long)threadIdx.x < n_bins - n_groups * W) {
        const unsigned key = cov_hist_key<E>((unsigned)src[n_groups * W + threadIdx.x]);
        cov_hist_add<CovHistIn<E>::has_skip>(h, key, 1u);
    }
    cov_hist_flush(lds, hist);
}

// the windows a width-1 / width-2 pass listed (value >= the code's limit): unordered, so no runs -- one LDS add per entry
__global__ __launch_bounds__(kCovHistThreads) void cov_hist_exc_kernel(const int32_t *__restrict__ val, long long n, unsigned long long *__restrict__ hist)
{
    __shared__ unsigned lds[kCovHistWaves][kCovHistBins];
    cov_hist_clear(lds);
    unsigned *h = lds[threadIdx.x >> 6];
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) atomicAdd(&h[cov_hist_bin((unsigned)val[i])], 1u);
    cov_hist_flush(lds, hist);
}

} // namespace raft
