// lift.hpp -- the record stream lifted onto the fragments (raft_hip_lift_overlaps_device / _host, include/raft_hip_lift.h): every record
// is cut at the fragment bounds of both reads and shifted into fragment coordinates, lift_rule.hpp's rule.  A stream expansion: count,
// prefix, fill, as filter.hpp is a compaction -- launch boundaries carry what crosses workgroups, no look-back, no workgroup waits for
// another (device_scan.hpp).  A tile is kLiftTile consecutive records, one workgroup step; a lane takes kStreamLaneRecords consecutive
// records with record_stream.hpp's lane loader.
//
//   * frag_digest_kernel (frag_ovl.hpp) checks the table and writes 16 bytes per read.
//   * lift_count_kernel streams the seven columns once, gathers the two digests of every record and walks the rule without writing:
//     a 64-bit count per tile, the first bad id, and the totals (records without an output, records with more than one, pairs dropped
//     under min_len, the most outputs of one record).
//   * device_scan.hpp's exclusive_scan over the tiles' counts: tile_base [n_tiles + 1], whose last element is n_out.  The host reads it.
//   * lift_fill_kernel ranks the lanes inside the tile -- the lane's count, the wave scan, the waves' totals through LDS -- and walks
//     the rule again to write the eight columns at tile_base[tile] + rank.  A record's pairs are RECOMPUTED, not stored; what the
//     count kernel does leave is ONE int32 per lane (its four records' outputs, lane_cnt: a byte per record), so that the fill kernel
//     walks once and not twice -- walking for the count as well cost 7 of 68 ms at the bench's size.
//
// The walk (lift_walk).  With one row on either read and neither side leaving it the record is answered from the two digests alone
// (lift_pair_whole: one output, no division, no CSR access).  Otherwise the touched rows of either read are a contiguous range --
// fb and fe do not descend within a read -- found with frag_first's searches, and the pairs are taken in lift_rule.hpp's order.  Every
// loop is bounded by the rows of the two reads.  Both kernels look at ctl[kLiftBadTable] first and leave when the table is broken.
#pragma once
#include "raft_types.hpp"
#include "wave.hpp"
#include "record_stream.hpp"
#include "frag_ovl.hpp"
#include "device_scan.hpp"
#include "lift_rule.hpp"

namespace raft {

constexpr int kLiftTile = kStreamThreads * kStreamLaneRecords;       // records of one workgroup step
static_assert(kLiftTile == 1024, "a tile is 1024 records (include/raft_hip_lift.h)");

// control words (unsigned long long each)
constexpr int kLiftFirstBad = 0;         // smallest record index with an id out of range; ~0 = none
constexpr int kLiftBadTable = 1;         // != 0: the fragment table is not what the header asks for
constexpr int kLiftNone = 2;             // records without an output
constexpr int kLiftCut = 3;              // records with more than one
constexpr int kLiftDropped = 4;          // pairs dropped under min_len
constexpr int kLiftMost = 5;             // the most outputs of one record
constexpr int kLiftCtlWords = 6;
static_assert(kLiftFirstBad == kFragFirstBad && kLiftBadTable == kFragBadTable, "frag_digest_kernel writes its verdict to ctl[kFragBadTable]");

inline long long lift_tiles(long long n_rec) { return (n_rec + kLiftTile - 1) / kLiftTile; }
inline unsigned lift_grid(long long n_tiles) { return (unsigned)(n_tiles < 1 ? 1 : (n_tiles > kStreamMaxBlocks ? kStreamMaxBlocks : n_tiles)); }

struct LiftArgs {
    const int32_t *qid, *qs, *qe, *tid, *ts, *te;
    const uint8_t *strand;
    long long n_rec, n_tiles;
    int32_t n_reads, min_len;
    const int32_t *fb, *fe;
    const FragDigest *digest;
    unsigned long long *ctl;
    long long *tile_cnt;                     // [n_tiles], written by the count kernel
    int32_t *lane_cnt;                       // [n_tiles * kStreamThreads]: the outputs of every lane's records, from the count kernel to the fill kernel
    const long long *tile_base;              // [n_tiles + 1], read by the fill kernel
    long long n_out;                         // the fill kernel's bound: tile_base[n_tiles]
    int32_t *out[6];                         // qfrag, qs, qe, tfrag, ts, te; any may be NULL
    uint8_t *rev;
    int32_t *src;
};

// the scan's loader: one sum, the tiles' counts
struct LiftTileCount {
    const long long *cnt;
    __device__ void operator()(long long i, long long (&v)[1]) const { v[0] = cnt[i]; }
};

// the touched rows [lo, hi) of the read with digest d under the side [s, e): d.n > 0 and the side meets the hull
__device__ __forceinline__ void lift_touched_range(const LiftArgs &A, const FragDigest d, int s, int e, int &lo, int &hi)
{
    lo = 0; hi = 1;
    if (d.n == 1) return;
    lo = frag_first<true>(A.fe + d.k0, 0, d.n, s);
    hi = frag_first<false>(A.fb + d.k0, lo, d.n, e);
}

// The outputs of one record with ids in range, emit(LiftRecord) for each in the rule's order; dropped gains the pairs under min_len.
template <class Emit>
__device__ __forceinline__ long long lift_walk(const LiftArgs &A, int q, int qs, int qe, int t, int ts, int te, bool rev, const FragDigest dq,
                                               const FragDigest dt, long long &dropped, Emit emit)
{
    LiftSides s;
    if (!lift_sides(q, qs, qe, t, ts, te, s)) return 0;
    const FragDigest da = s.swap ? dt : dq, db = s.swap ? dq : dt;
    // (coordinates are int32: the canonical sides fit)
    const int as = (int)s.as, ae = (int)s.ae, bs = (int)s.bs, be = (int)s.be;
    if (da.n == 0 || db.n == 0 || da.y <= as || da.x >= ae || db.y <= bs || db.x >= be) return 0;     // (outside a hull: no pair of touched rows)
    LiftPair p;
    if (da.n == 1 && db.n == 1 && as >= da.x && ae <= da.y && bs >= db.x && be <= db.y) {
        if (!lift_pair_whole(s, da.x, db.x, A.min_len, p)) { ++dropped; return 0; }
        emit(lift_record(s.swap, da.k0, db.k0, p));
        return 1;
    }
    int li, hi, lj, hj;
    lift_touched_range(A, da, as, ae, li, hi);
    lift_touched_range(A, db, bs, be, lj, hj);
    long long n = 0;
    for (int i = li; i < hi; ++i) {
        const int fb_a = da.n == 1 ? da.x : A.fb[da.k0 + i], fe_a = da.n == 1 ? da.y : A.fe[da.k0 + i];
        for (int j = lj; j < hj; ++j) {
            const int fb_b = db.n == 1 ? db.x : A.fb[db.k0 + j], fe_b = db.n == 1 ? db.y : A.fe[db.k0 + j];
            if (lift_pair(s, fb_a, fe_a, fb_b, fe_b, rev, A.min_len, p)) { emit(lift_record(s.swap, (long long)da.k0 + i, (long long)db.k0 + j, p)); ++n; }
            else ++dropped;
        }
    }
    return n;
}

// a lane's records, their strand bytes and the digests of their reads; ok[i]: the record is there and both ids name a read
struct LiftLane {
    LaneRecords r;
    unsigned strand;
    FragDigest dq[kStreamLaneRecords], dt[kStreamLaneRecords];
    bool ok[kStreamLaneRecords];
};

// kCheck: the count kernel's load, which keeps the first bad id
template <bool kVec, bool kCheck>
__device__ __forceinline__ void lift_load(const LiftArgs &A, long long first, LiftLane &L)
{
    constexpr int R = kStreamLaneRecords;
    stream_load_records<kVec>(A.qid, A.qs, A.qe, A.tid, A.ts, A.te, first, A.n_rec, true, L.r);
    L.strand = stream_load_bytes<kVec>(A.strand, first, A.n_rec);
    const unsigned n_reads = (unsigned)A.n_reads;
#pragma unroll
    for (int i = 0; i < R; ++i) {                           // the gathers of the lane's eight sides first, all in flight together
        const bool have = first + i < A.n_rec;
        if (kCheck) {
            const IdsValid v = stream_check_ids(have, first + i, L.r.q[i], L.r.t[i], n_reads, &A.ctl[kLiftFirstBad]);
            L.ok[i] = v.q && v.t;
        } else L.ok[i] = have && (unsigned)L.r.q[i] < n_reads && (unsigned)L.r.t[i] < n_reads;
        L.dq[i] = L.dt[i] = FragDigest{0, 0, 0, 0};
        if (L.ok[i] && L.r.q[i] != L.r.t[i]) {
            L.dq[i] = A.digest[L.r.q[i]];
            L.dt[i] = A.digest[L.r.t[i]];
        }
    }
}

template <class Emit>
__device__ __forceinline__ long long lift_walk_lane(const LiftArgs &A, const LiftLane &L, int i, long long &dropped, Emit emit)
{
    if (!L.ok[i]) return 0;
    return lift_walk(A, L.r.q[i], L.r.qs[i], L.r.qe[i], L.r.t[i], L.r.ts[i], L.r.te[i], (L.strand >> (8 * i) & 0xffu) != 0, L.dq[i], L.dt[i], dropped, emit);
}

struct LiftNoEmit { __device__ void operator()(const LiftRecord &) const {} };

// kVec: the six columns begin on 16-byte lines and the strand bytes on a 4-byte one
template <bool kVec>
__global__ __launch_bounds__(kStreamThreads) void lift_count_kernel(LiftArgs A)
{
    constexpr int R = kStreamLaneRecords;
    __shared__ long long wave_cnt[kStreamThreads / kWave];
    if (A.ctl[kLiftBadTable]) return;                       // (uniform: the digest kernel's verdict, written before this launch)
    const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    unsigned tot[2] = {0, 0};                               // this lane's records without an output / with more than one
    long long dropped = 0, most = 0;
    // (the loop's bound is the workgroup's: every lane takes part in the scans and the barriers)
    for (long long tile = blockIdx.x; tile < A.n_tiles; tile += gridDim.x) {
        const long long rec0 = tile * kLiftTile + (long long)tid * R;        // (at or beyond n_rec: a lane without records)
        LiftLane L;
        lift_load<kVec, true>(A, rec0, L);
        long long mine = 0;
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const long long n = lift_walk_lane(A, L, i, dropped, LiftNoEmit());
            mine += n;
            if (rec0 + i < A.n_rec) { tot[0] += n == 0 ? 1 : 0; tot[1] += n > 1 ? 1 : 0; }
            most = n > most ? n : most;
        }
        A.lane_cnt[tile * kStreamThreads + tid] = (int32_t)mine;             // (n_out < 2^31 - 1 wherever the fill kernel runs)
        const long long in_wave = wave_reduce_add64(mine);
        if (lane == 0) wave_cnt[wid] = in_wave;
        __syncthreads();
        if (tid == 0) {
            long long total = 0;
#pragma unroll
            for (int w = 0; w < kStreamThreads / kWave; ++w) total += wave_cnt[w];
            A.tile_cnt[tile] = total;
        }
        __syncthreads();
    }
    wave_flush_totals(tot, &A.ctl[kLiftNone], lane);
    const long long wave_dropped = wave_reduce_add64(dropped);
#pragma unroll
    for (int x = 1; x < kWave; x <<= 1) {
        const long long o = __shfl_xor(most, x, kWave);
        most = o > most ? o : most;
    }
    if (lane == 0) {
        if (wave_dropped) atomicAdd(&A.ctl[kLiftDropped], (unsigned long long)wave_dropped);
        if (most) atomicMax(&A.ctl[kLiftMost], (unsigned long long)most);
    }
}

// writes one output at `at` and moves on; nothing behind n_out (the count kernel's total) is ever written
struct LiftStore {
    const LiftArgs &A;
    long long at;
    int32_t record;
    uint8_t rev;
    __device__ void operator()(const LiftRecord &o)
    {
        if (at < A.n_out) {
            const int32_t v[6] = {o.qfrag, o.qs, o.qe, o.tfrag, o.ts, o.te};
#pragma unroll
            for (int k = 0; k < 6; ++k)
                if (A.out[k]) A.out[k][at] = v[k];
            if (A.rev) A.rev[at] = rev;
            if (A.src) A.src[at] = record;
        }
        ++at;
    }
};
struct LiftStoreRef {                                       // (lift_walk takes its emit by value)
    LiftStore *s;
    __device__ void operator()(const LiftRecord &o) const { (*s)(o); }
};

template <bool kVec>
__global__ __launch_bounds__(kStreamThreads) void lift_fill_kernel(LiftArgs A)
{
    constexpr int R = kStreamLaneRecords;
    __shared__ long long wave_cnt[kStreamThreads / kWave];
    if (A.ctl[kLiftBadTable]) return;
    const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    for (long long tile = blockIdx.x; tile < A.n_tiles; tile += gridDim.x) {
        const long long base = A.tile_base[tile];
        if (A.tile_base[tile + 1] == base) continue;        // (uniform: a tile without an output)
        const long long rec0 = tile * kLiftTile + (long long)tid * R;
        const long long mine = A.lane_cnt[tile * kStreamThreads + tid];
        const long long incl = wave_incl_scan_add64(mine);
        if (lane == kWave - 1) wave_cnt[wid] = incl;
        __syncthreads();
        long long before = 0;
#pragma unroll
        for (int w = 0; w < kStreamThreads / kWave; ++w) before += w < wid ? wave_cnt[w] : 0;
        __syncthreads();
        if (mine) {                                         // (a lane without an output loads nothing)
            LiftLane L;
            lift_load<kVec, false>(A, rec0, L);
            long long dropped = 0;
            LiftStore st{A, base + before + incl - mine, 0, 0};
#pragma unroll
            for (int i = 0; i < R; ++i) {
                st.record = (int32_t)(rec0 + i);
                st.rev = (L.strand >> (8 * i) & 0xffu) != 0 ? 1 : 0;
                lift_walk_lane(A, L, i, dropped, LiftStoreRef{&st});
            }
        }
    }
}

} // namespace raft
