// record_stream.hpp -- what the kernels that stream the record columns once share (census.hpp, ovl_class.hpp, repeat_stats.hpp,
// frag_ovl.hpp, ovl_ends.hpp, best_ovl.hpp; filter.hpp takes the lane loader): the launch shape, the lane's loads and stores, the
// loop over a wave's lane groups, the first-bad-record rule, and the join of equal neighbouring ids before anything leaves the wave.
//
//   * shape: a lane takes kStreamLaneRecords consecutive records per step -- one 16-byte load per int32 column, one 32-bit access per
//     byte column --, a workgroup kStreamThreads lanes, the grid at most kStreamMaxBlocks workgroups with a grid-stride loop beyond.
//     A stream whose columns do not begin on a 16-byte line (byte columns: a 4-byte one), and the records behind the last whole
//     group, take element accesses (kVec = false is the first; the second is looked at per lane).
//   * an id outside [0, n_reads) in either column: the smallest such record index is kept in control word 0 (atomicMin); what the
//     record then counts for is the kernel's business.
//   * the join (join_runs): a stream is mostly sorted runs of one query id, so one global atomic per record would queue up on one
//     address.  Equal neighbouring ids are joined within the lane and then across the wave -- a segmented scan over the lanes' last
//     runs: a lane whose records are all on the id the lane before ended with carries that run on --, and the run's value is emitted
//     once per run and wave.  The value, how two are combined, and what emitting means are the caller's: a count and atomicAdd
//     (census), packed counts (ovl_class, repeat_stats, ovl_ends), a pair of keys under max (best_ovl).
#pragma once
#include "raft_types.hpp"
#include "wave.hpp"

namespace raft {

constexpr int kStreamThreads = 256;
constexpr int kStreamLaneRecords = 4;        // consecutive records of one lane per step: one 16-byte load per column
constexpr int kStreamMaxBlocks = 2048;       // eight workgroups on each of the 256 CUs, grid-stride beyond
constexpr int kStreamWaveRecords = kStreamLaneRecords * kWave;       // records of one wave per step: what a join combines at most

inline unsigned stream_grid(long long n_rec)
{
    const long long per_step = (long long)kStreamThreads * kStreamLaneRecords;       // records one workgroup takes per step
    const long long want = (n_rec + per_step - 1) / per_step;
    return (unsigned)(want < 1 ? 1 : (want > kStreamMaxBlocks ? kStreamMaxBlocks : want));
}

// the lane's records of one column, `fill` behind n_rec
template <bool kVec>
__device__ __forceinline__ void stream_load(const int32_t *col, long long first, long long n_rec, int fill, int (&v)[kStreamLaneRecords])
{
    if (kVec && first + kStreamLaneRecords <= n_rec) {
        const int4 q = *reinterpret_cast<const int4 *>(col + first);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int i = 0; i < kStreamLaneRecords; ++i) v[i] = first + i < n_rec ? col[first + i] : fill;
    }
}

// ... of the six columns, -1 behind n_rec; ts / te only where the kernel looks at them (they may be NULL otherwise)
struct LaneRecords { int q[kStreamLaneRecords], t[kStreamLaneRecords], qs[kStreamLaneRecords], qe[kStreamLaneRecords], ts[kStreamLaneRecords], te[kStreamLaneRecords]; };

template <bool kVec>
__device__ __forceinline__ void stream_load_records(const int32_t *qid, const int32_t *qs, const int32_t *qe, const int32_t *tid, const int32_t *ts,
                                                    const int32_t *te, long long first, long long n_rec, bool targets, LaneRecords &r)
{
    stream_load<kVec>(qid, first, n_rec, -1, r.q);
    stream_load<kVec>(tid, first, n_rec, -1, r.t);
    stream_load<kVec>(qs, first, n_rec, -1, r.qs);
    stream_load<kVec>(qe, first, n_rec, -1, r.qe);
    if (targets) {
        stream_load<kVec>(ts, first, n_rec, -1, r.ts);
        stream_load<kVec>(te, first, n_rec, -1, r.te);
    }
}

// the lane's four bytes of a byte column as one word, byte i at bits 8 i (0 behind n_rec), and four such bytes back out
static_assert(kStreamLaneRecords == 4, "a lane's bytes of a byte column are one 32-bit word");

template <bool kVec>
__device__ __forceinline__ unsigned stream_load_bytes(const uint8_t *col, long long first, long long n_rec)
{
    if (kVec && first + kStreamLaneRecords <= n_rec) return *reinterpret_cast<const unsigned *>(col + first);
    unsigned word = 0;
#pragma unroll
    for (int i = 0; i < kStreamLaneRecords; ++i)
        if (first + i < n_rec) word |= (unsigned)col[first + i] << (8 * i);
    return word;
}

template <bool kVec>
__device__ __forceinline__ void stream_store_bytes(uint8_t *col, long long first, long long n_rec, unsigned word)
{
    if (kVec && first + kStreamLaneRecords <= n_rec) *reinterpret_cast<unsigned *>(col + first) = word;
    else {
#pragma unroll
        for (int i = 0; i < kStreamLaneRecords; ++i)
            if (first + i < n_rec) col[first + i] = (uint8_t)(word >> (8 * i));
    }
}

// body(first) once per lane group of the stream, grid-stride.  The loop's bound is the wave's, not the lane's: every lane of a wave
// enters the body -- a lane whose `first` is at or beyond n_rec as a lane without records --, because join_runs shuffles across the
// wave and needs EXEC all ones.
template <class Body>
__device__ __forceinline__ void stream_for_each_group(long long n_rec, int lane, Body body)
{
    const long long n_groups = (n_rec + kStreamLaneRecords - 1) / kStreamLaneRecords;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long g0 = (long long)blockIdx.x * blockDim.x + ((int)threadIdx.x & ~(kWave - 1)); g0 < n_groups; g0 += stride) {
        body((g0 + lane) * kStreamLaneRecords);            // (at or beyond n_rec: a lane without records)
    }
}

// Which of the two ids of record `rec` name a read.  A record that is there (`have`) with either id outside [0, n_reads) is kept as
// the first bad record when it is the smallest: ctl[0].
struct IdsValid { bool q, t; };

__device__ __forceinline__ IdsValid stream_check_ids(bool have, long long rec, int q, int t, unsigned n_reads, unsigned long long *ctl)
{
    const IdsValid v{have && (unsigned)q < n_reads, have && (unsigned)t < n_reads};
    if (have && !(v.q && v.t)) atomicMin(ctl, (unsigned long long)rec);
    return v;
}

// flags[r] |= bits.  A contained read is contained by many records (ten a side on a human set), neighbours in the stream: the word is
// looked at first and the atomic goes out only while a bit is missing.  Bits are only ever set, so a stale look costs an atomic, never a bit.
__device__ __forceinline__ void ovl_flag(unsigned *word, unsigned bits)
{
    if ((__atomic_load_n(word, __ATOMIC_RELAXED) & bits) != bits) atomicOr(word, bits);
}

// a join's value from d lanes below (a value of several words overloads this with one shuffle per word)
__device__ __forceinline__ unsigned join_shfl_up(unsigned v, int d) { return __shfl_up(v, d, kWave); }
__device__ __forceinline__ unsigned long long join_shfl_up(unsigned long long v, int d) { return __shfl_up(v, d, kWave); }

// emit(id, combine over the lane's records with that id of w), for every lane of the wave: equal neighbouring ids are joined first,
// within the lane and across the wave, so that a run of one id within the wave is emitted once.  emit decides what is worth sending:
// it looks at the value before it uses the id (a record that adds nothing may come with any id, one out of range included).
// combine is associative.  EXEC must be all ones.
template <class V, class Combine, class Emit>
__device__ __forceinline__ void join_runs(const int (&id)[kStreamLaneRecords], const V (&w)[kStreamLaneRecords], int lane, Combine combine, Emit emit)
{
    int cur = id[0];
    V n = w[0], head{};
    bool uniform = true;
#pragma unroll
    for (int i = 1; i < kStreamLaneRecords; ++i) {
        if (id[i] == cur) n = combine(n, w[i]);
        else {
            if (uniform) { head = n; uniform = false; }
            else emit(cur, n);                             // a run that touches neither end of the lane
            cur = id[i]; n = w[i];
        }
    }
    // the lane's last run (cur, n) opens a segment unless the lane is one run that carries on what the lane before ended with
    const int prev_tail = __shfl_up(cur, 1, kWave);
    const bool joins = lane > 0 && id[0] == prev_tail;
    V x = n;
    int f = (!uniform || !joins) ? 1 : 0;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const V xo = join_shfl_up(x, d);
        const int fo = __shfl_up(f, d, kWave);
        if (lane >= d && !f) { x = combine(x, xo); f = fo; }
    }
    const V before = join_shfl_up(x, 1);                   // the open run as the lane before left it
    const int next_joins = __shfl_down(joins ? 1 : 0, 1, kWave);
    if (!uniform) emit(id[0], joins ? combine(head, before) : head);
    if (lane == kWave - 1 || !next_joins) emit(cur, x);
}

// the join of counts: combine is +
struct JoinAdd {
    template <class V> __device__ __forceinline__ V operator()(V a, V b) const { return a + b; }
};

} // namespace raft
