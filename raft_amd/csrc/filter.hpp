// filter.hpp -- which records of a stream go into a job at all (raft_hip_filter_overlaps_device / _host, include/raft_hip_flt.h):
//
//     identity_ok = P == 0 || (block > 0 && matches >= 0 && (int64)matches * 1000 >= (int64)P * block)
//     span_ok     = L == 0 || ((int64)qe - qs >= L && (int64)te - ts >= L)
//     keep        = identity_ok && span_ok
//
// and the kept records of the six columns, in their order, in six other arrays: a stream compaction.  Count, prefix, scatter, as
// low_cov.hpp and finalize.hpp do it -- launch boundaries carry what crosses workgroups: no look-back, no workgroup waits for another
// (device_scan.hpp: the look-back lost here at full size).  A tile is kFltTile consecutive records, one workgroup step; a lane takes
// kFltLaneRecords consecutive records with record_stream.hpp's lane loader (stream_load: one 16-byte load per column, 4-byte loads
// for a column that is not 16-byte aligned and behind the last whole group).
//
//   * flt_flag_kernel streams matches, block (only when P > 0), qs, qe, ts, te ONCE and evaluates the rule.  A lane's four keep bits
//     are ORed across 16 lanes by shuffles into one 64-bit word of the bitmap `bits` (bit i of word w: record 64 w + i; whole tiles
//     are written, bits behind n_rec are 0).  The tile's kept count goes into tile_cnt; the two below_* totals go out with one
//     atomic per wave, the smallest kept index with one atomicMin per wave.
//   * device_scan.hpp's exclusive_scan over tile_cnt: tile_base [n_tiles + 1], whose last element is n_kept.
//   * flt_scatter_kernel reads the bitmap instead of the rule (the quality columns are not read again), ranks a lane's kept records
//     inside the tile -- popcount, wave scan, the waves' totals through LDS -- and copies the six values of every kept record to
//     tile_base[tile] + rank: a tile's stores are one contiguous range per column.  A lane without a kept record loads nothing.
//     On the way every kept record other than the first kept one (known from the flag kernel) is compared with that record's mirror:
//     the symmetric flag of the kept stream (chop.hpp:171-184), without another pass.
#pragma once
#include "raft_types.hpp"
#include "wave.hpp"
#include "record_stream.hpp"
#include "census.hpp"
#include "device_scan.hpp"

namespace raft {

constexpr int kFltThreads = 256;
constexpr int kFltLaneRecords = kStreamLaneRecords;                  // stream_load's group (record_stream.hpp)
constexpr int kFltTile = kFltThreads * kFltLaneRecords;              // records of one workgroup step
constexpr int kFltTileWords = kFltTile / 64;                         // bitmap words of a tile
constexpr int kFltWordLanes = 64 / kFltLaneRecords;                  // lanes whose bits make one word
constexpr int kFltMaxBlocks = 2048;                                  // eight workgroups on each of the 256 CUs, grid-stride beyond
static_assert(kFltLaneRecords == kStreamLaneRecords, "stream_load fills kStreamLaneRecords values");
static_assert(kFltLaneRecords == 4 && kFltTile == 1024 && kFltWordLanes == 16, "a nibble per lane, a word per 16 lanes");

// control words of one call: [0] the first kept record (all ones: none; the flag kernel takes the minimum), [1] below identity,
// [2] below span, [3] the kept stream is symmetric
constexpr int kFltFirst = 0, kFltBelowIdentity = 1, kFltBelowSpan = 2, kFltSymmetric = 3;
constexpr int kFltCtlWords = 4;

inline long long flt_tiles(long long n_rec) { return (n_rec + kFltTile - 1) / kFltTile; }
inline unsigned flt_grid(long long n_tiles) { return (unsigned)(n_tiles < 1 ? 1 : (n_tiles > kFltMaxBlocks ? kFltMaxBlocks : n_tiles)); }

struct FltFlagArgs {
    const int32_t *qs, *qe, *ts, *te, *matches, *block;
    long long n_rec, n_tiles;
    int32_t permille, min_span;
    unsigned long long *bits;                // [n_tiles * kFltTileWords]
    int32_t *tile_cnt;                       // [n_tiles]
    unsigned long long *ctl;
};

// the scan's loader: one sum, the tiles' counts
struct FltTileCount {
    const int32_t *cnt;
    __device__ void operator()(long long i, long long (&v)[1]) const { v[0] = cnt[i]; }
};

// kVec: every column read begins on a 16-byte line.  kIdent: P > 0 (otherwise matches / block are not read and may be NULL).
template <bool kVec, bool kIdent>
__global__ __launch_bounds__(kFltThreads) void flt_flag_kernel(FltFlagArgs A)
{
    constexpr int R = kFltLaneRecords;
    __shared__ int wave_cnt[kFltThreads / kWave];
    const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    const long long P = A.permille, L = A.min_span;
    int below_identity = 0, below_span = 0;                 // this lane's, over all its tiles (n_rec / grid < 2^31 per lane)
    unsigned long long first = ~0ull;
    // (the loop's bound is the workgroup's: every lane takes part in the shuffles, the scans and the barriers)
    for (long long tile = blockIdx.x; tile < A.n_tiles; tile += gridDim.x) {
        const long long rec0 = tile * kFltTile + (long long)tid * R;          // (at or beyond n_rec: a lane without records)
        int a[R], b[R], s[R], e[R], m[R], d[R];
        stream_load<kVec>(A.qs, rec0, A.n_rec, 0, a);
        stream_load<kVec>(A.qe, rec0, A.n_rec, 0, b);
        stream_load<kVec>(A.ts, rec0, A.n_rec, 0, s);
        stream_load<kVec>(A.te, rec0, A.n_rec, 0, e);
        if (kIdent) {
            stream_load<kVec>(A.matches, rec0, A.n_rec, 0, m);
            stream_load<kVec>(A.block, rec0, A.n_rec, 0, d);
        }
        unsigned keep = 0;
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const bool have = rec0 + i < A.n_rec;
            bool identity_ok = true;
            if (kIdent) identity_ok = d[i] > 0 && m[i] >= 0 && (long long)m[i] * 1000 >= P * (long long)d[i];
            const bool span_ok = L == 0 || ((long long)b[i] - a[i] >= L && (long long)e[i] - s[i] >= L);
            below_identity += have && !identity_ok ? 1 : 0;
            below_span += have && !span_ok ? 1 : 0;
            keep |= (have && identity_ok && span_ok ? 1u : 0u) << i;
        }
        if (keep && first == ~0ull) first = (unsigned long long)(rec0 + (__ffs((int)keep) - 1));   // (tiles ascend: the lane's first hit is its smallest)
        // the word of this lane's 16: every nibble at its place, ORed together
        unsigned long long word = (unsigned long long)keep << (R * (lane & (kFltWordLanes - 1)));
#pragma unroll
        for (int x = 1; x < kFltWordLanes; x <<= 1) word |= (unsigned long long)__shfl_xor((long long)word, x, kWave);
        if ((lane & (kFltWordLanes - 1)) == 0) A.bits[tile * kFltTileWords + tid / kFltWordLanes] = word;
        const int in_wave = wave_reduce_add(__popc(keep));
        if (lane == 0) wave_cnt[wid] = in_wave;
        __syncthreads();
        if (tid == 0) {
            int total = 0;
#pragma unroll
            for (int w = 0; w < kFltThreads / kWave; ++w) total += wave_cnt[w];
            A.tile_cnt[tile] = total;
        }
        __syncthreads();
    }
    const int wave_identity = wave_reduce_add(below_identity), wave_span = wave_reduce_add(below_span);
#pragma unroll
    for (int x = 1; x < kWave; x <<= 1) {
        const unsigned long long o = (unsigned long long)__shfl_xor((long long)first, x, kWave);
        first = o < first ? o : first;
    }
    if (lane == 0) {
        if (wave_identity) atomicAdd(&A.ctl[kFltBelowIdentity], (unsigned long long)wave_identity);
        if (wave_span) atomicAdd(&A.ctl[kFltBelowSpan], (unsigned long long)wave_span);
        if (first != ~0ull) atomicMin(&A.ctl[kFltFirst], first);
    }
}

struct FltScatterArgs {
    const int32_t *in[6];                    // qid, qs, qe, tid, ts, te
    int32_t *out[6];                         // [n_kept] at least
    long long n_rec, n_tiles;
    const unsigned long long *bits;
    const long long *tile_base;              // [n_tiles + 1]
    unsigned long long *ctl;
};

template <bool kVec>
__global__ __launch_bounds__(kFltThreads) void flt_scatter_kernel(FltScatterArgs A)
{
    constexpr int R = kFltLaneRecords;
    __shared__ int wave_cnt[kFltThreads / kWave];
    __shared__ int mirror[6];                               // the first kept record, sides exchanged: tid, ts, te, qid, qs, qe
    const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    const unsigned long long first = A.ctl[kFltFirst];      // (written by the launch before)
    if (first == ~0ull) return;                             // nothing is kept
    if (tid < 6) mirror[tid] = A.in[(tid + 3) % 6][first];
    __syncthreads();
    int want[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) want[k] = mirror[k];
    bool mirrored = false;
    for (long long tile = blockIdx.x; tile < A.n_tiles; tile += gridDim.x) {
        const long long rec0 = tile * kFltTile + (long long)tid * R;
        const unsigned keep = (unsigned)(A.bits[tile * kFltTileWords + tid / kFltWordLanes] >> (R * (lane & (kFltWordLanes - 1)))) & ((1u << R) - 1u);
        const int mine = __popc(keep);
        const int incl = wave_incl_scan_add(mine);
        if (lane == kWave - 1) wave_cnt[wid] = incl;
        __syncthreads();
        int before = 0;
#pragma unroll
        for (int w = 0; w < kFltThreads / kWave; ++w) before += w < wid ? wave_cnt[w] : 0;
        __syncthreads();
        if (keep) {                                         // (bits behind n_rec are 0: a kept record exists)
            long long at = A.tile_base[tile] + before + incl - mine;
            int v[6][R];
#pragma unroll
            for (int k = 0; k < 6; ++k) stream_load<kVec>(A.in[k], rec0, A.n_rec, 0, v[k]);
#pragma unroll
            for (int i = 0; i < R; ++i)
                if (keep >> i & 1u) {
                    bool same = (unsigned long long)(rec0 + i) != first;
#pragma unroll
                    for (int k = 0; k < 6; ++k) {
                        A.out[k][at] = v[k][i];
                        same = same && v[k][i] == want[k];
                    }
                    mirrored = mirrored || same;
                    ++at;
                }
        }
    }
    if (mirrored) atomicOr(&A.ctl[kFltSymmetric], 1ull);
}

} // namespace raft
