// unitig.hpp -- the unitigs of the best overlap graph (raft_hip_unitigs_device / _host, include/raft_hip_utg.h): list ranking over the
// half-edges of unitig_rule.hpp, then one pass per read that turns the ranks into the layout.
//
// Kernels, none of which waits for another workgroup (one launch per round, the host between the ranking and the rest):
//   * utg_init_kernel: a lane per read runs the consistency rule on its two ends (atomicMin of the first bad read; a bad end is
//     treated as no edge, so every pointer that is ever followed lies in range) and writes the state of its two half-edges, 64 B
//     that one lane owns.  With `cut` given, the edge that enters 2 * M + 1 and the one that leaves 2 * M + 0 are left out for every
//     read M flagged there: the cycle whose smallest read is M becomes a path that starts at M on '+'.
//   * utg_jump_kernel: one round of pointer jumping from one half of the state into the other (ping-pong: a round reads only what
//     the round before wrote, so the result is a function of the input alone).  A state is 32 B on a 32-byte line -- next, the
//     count of steps, the 64-bit sum of weights, the last half-edge reached, the smallest read seen -- so a gather touches one
//     sector.  A half-edge whose walk has ended (next < 0) gathers nothing.  The last round counts the half-edges still under way:
//     those lie on cycles, and their minimum is the cycle's smallest read.
//   * utg_mark_kernel (only if that count is not 0): cut[r] = read r is the smallest of a cycle.
//   * utg_place_kernel: a lane per read derives start read, index, offset, orientation from its two half-edges; a start read also
//     the unitig's size and length.
//   * one exclusive scan (device_scan.hpp, K = 2) over the reads: "is a start" gives the dense ids in the order of the start reads,
//     "size if a start" gives utg_off.
//   * utg_emit_kernel: a lane per read gathers its start's two prefixes and writes unitig, index and its slot of `order`; a start
//     writes its unitig's row; the totals are kept per lane and leave with one atomic per wave and total.
#pragma once
#include "wave.hpp"
#include "unitig_rule.hpp"

namespace raft {

constexpr int kUtgThreads = 256;
constexpr int kUtgMaxBlocks = 2048;          // eight workgroups on each of the 256 CUs, grid-stride beyond
// control words: the first bad read, the half-edges on cycles, then the totals of utg_emit_kernel
constexpr int kUtgCtlCycle = 1, kUtgCtlTotals = 2;
constexpr int kUtgSkipped = 0, kUtgUnitigs = 1, kUtgSingletons = 2, kUtgCircular = 3, kUtgTotalLength = 4, kUtgLongestReads = 5, kUtgLongestLength = 6;
constexpr int kUtgTotals = 7, kUtgCtlWords = kUtgCtlTotals + kUtgTotals;

struct alignas(32) UtgState {
    int32_t next;                            // the half-edge the walk has got to, kUtgNil once it has ended
    int32_t cnt;                             // steps so far
    long long w;                             // their weights
    int32_t last;                            // the last half-edge reached (the half-edge itself before the first step)
    int32_t min;                             // the smallest read seen
    long long pad;
};
static_assert(sizeof(UtgState) == 32, "one state, one 32-byte line");

// per read, what utg_place_kernel leaves for the scan and utg_emit_kernel: {start read (-1: SKIPPED), index, size if a start else 0, 0}
using UtgPlace = int4;

inline unsigned utg_grid(long long n) { return (unsigned)(n < 1 ? 1 : ((n + kUtgThreads - 1) / kUtgThreads > kUtgMaxBlocks ? kUtgMaxBlocks : (n + kUtgThreads - 1) / kUtgThreads)); }

__global__ __launch_bounds__(kUtgThreads) void utg_init_kernel(int32_t n_reads, const int32_t *__restrict__ len, const int32_t *__restrict__ partner,
                                                               const int32_t *__restrict__ span, const uint8_t *__restrict__ flags,
                                                               const uint8_t *__restrict__ cut, UtgState *__restrict__ state,
                                                               unsigned long long *__restrict__ ctl)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_reads; i += stride) {
        const int32_t r = (int32_t)i;
        bool bad = false;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int32_t h = utg_half(r, e);
            UtgState s{kUtgNil, 0, 0, h, r, 0};
            if (!utg_end_ok(n_reads, len, partner, span, flags, r, e)) bad = true;
            else {
                int32_t nx = utg_succ(partner, flags, r, e);
                if (nx != kUtgNil && cut && ((e == 0 && cut[r]) || (utg_end(nx) == 1 && cut[utg_read(nx)]))) nx = kUtgNil;
                if (nx != kUtgNil) {
                    const int32_t p = utg_read(nx);
                    s = UtgState{nx, 1, utg_weight(len, partner, span, r, e), nx, p < r ? p : r, 0};
                }
            }
            state[h] = s;
        }
        if (bad) atomicMin(ctl, (unsigned long long)r);
    }
}

template <bool kCount>
__global__ __launch_bounds__(kUtgThreads) void utg_jump_kernel(const UtgState *__restrict__ in, UtgState *__restrict__ out, long long n_half,
                                                               unsigned long long *__restrict__ ctl)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    unsigned open = 0;
    for (long long h = (long long)blockIdx.x * blockDim.x + threadIdx.x; h < n_half; h += stride) {
        UtgState s = in[h];
        if (s.next >= 0) {
            const UtgState t = in[s.next];
            s.cnt += t.cnt; s.w += t.w; s.last = t.last;
            s.min = t.min < s.min ? t.min : s.min;
            s.next = t.next;
        }
        out[h] = s;
        if (kCount && s.next >= 0) open += 1;
    }
    if (kCount) {                                          // (all lanes are back together here)
        const unsigned total = (unsigned)wave_reduce_add((int)open);
        if (((int)threadIdx.x & (kWave - 1)) == 0 && total) atomicAdd(&ctl[kUtgCtlCycle], (unsigned long long)total);
    }
}

// One ranking on stream st: the init kernel, then `rounds` rounds from one half of the state into the other, beginning with half[0].
// Returns the half the last round wrote; with `count` the last round counts the half-edges still under way.  The kernels it
// launched are added to *launches.  (unitig_lib.hip and graph_clean_lib.hip rank with it.)
inline UtgState *utg_rank(hipStream_t st, int32_t n_reads, const int32_t *len, const int32_t *partner, const int32_t *span, const uint8_t *flags,
                          const uint8_t *cut, UtgState *const (&half)[2], unsigned long long *ctl, int rounds, bool count, int64_t *launches)
{
    const long long n_half = 2 * (long long)n_reads;
    hipLaunchKernelGGL(utg_init_kernel, dim3(utg_grid(n_reads)), dim3(kUtgThreads), 0, st, n_reads, len, partner, span, flags, cut, half[0], ctl);
    const dim3 grid(utg_grid(n_half)), block(kUtgThreads);
    for (int k = 0; k < rounds; ++k) {
        if (count && k == rounds - 1) hipLaunchKernelGGL(utg_jump_kernel<true>, grid, block, 0, st, half[k & 1], half[(k + 1) & 1], n_half, ctl);
        else hipLaunchKernelGGL(utg_jump_kernel<false>, grid, block, 0, st, half[k & 1], half[(k + 1) & 1], n_half, ctl);
    }
    *launches += 1 + rounds;
    return half[rounds & 1];
}

__global__ __launch_bounds__(kUtgThreads) void utg_mark_kernel(const UtgState *__restrict__ state, int32_t n_reads, uint8_t *__restrict__ cut)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += stride) {
        const UtgState s = state[2 * r + 1];
        cut[r] = (s.next >= 0 && s.min == (int32_t)r) ? 1 : 0;
    }
}

__global__ __launch_bounds__(kUtgThreads) void utg_place_kernel(const UtgState *__restrict__ state, int32_t n_reads, const int32_t *__restrict__ len,
                                                                const int32_t *__restrict__ span, const uint8_t *__restrict__ flags,
                                                                const uint8_t *__restrict__ cut, UtgPlace *__restrict__ place,
                                                                long long *__restrict__ offset, long long *__restrict__ ulen, uint8_t *__restrict__ orient)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += stride) {
        UtgPlace pl = make_int4(-1, -1, 0, 0);
        long long off = 0, length = 0;
        int back = 0;
        if (!utg_skipped(flags[r])) {
            const UtgState s[2] = {state[2 * r], state[2 * r + 1]};
            // the walk from the start enters through the end whose own walk ends at the start read: the terminal with the smaller id
            // (both are the read itself where it stands alone: '+')
            back = utg_read(s[0].last) <= utg_read(s[1].last) ? 0 : 1;
            const UtgState &b = s[back], &f = s[1 - back];
            pl.x = utg_read(b.last); pl.y = b.cnt; off = b.w;
            if (b.cnt == 0) {                              // the start: the size and the length of its unitig
                pl.z = f.cnt + 1;
                length = (long long)utg_len(len[r]) + f.w - ((cut && cut[r]) ? (long long)span[2 * r] : 0);
            }
        }
        place[r] = pl; offset[r] = off; ulen[r] = length; orient[r] = (uint8_t)back;
    }
}

// the scan's elements: {is a start, the unitig's size if it is}
struct UtgStartLoader {
    const UtgPlace *place;
    __device__ void operator()(long long i, long long (&v)[2]) const
    {
        const int size = place[i].z;
        v[0] = size > 0 ? 1 : 0; v[1] = size;
    }
};

__device__ __forceinline__ long long utg_wave_max(long long v)
{
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) {
        const long long o = __shfl_xor(v, d, kWave);
        v = o > v ? o : v;
    }
    return v;
}

struct UtgOut {
    int32_t *unitig, *index, *order;         // [n_reads] each
    long long *utg_off;                      // [n_reads + 1]
    int32_t *utg_reads; long long *utg_length; uint8_t *utg_circular;   // [n_reads] each
};

__global__ __launch_bounds__(kUtgThreads) void utg_emit_kernel(const UtgPlace *__restrict__ place, int32_t n_reads, const long long *__restrict__ ulen,
                                                               const uint8_t *__restrict__ cut, const long long *__restrict__ start_id,
                                                               const long long *__restrict__ start_off, UtgOut out, unsigned long long *__restrict__ ctl)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    const int lane = (int)threadIdx.x & (kWave - 1);
    unsigned skipped = 0, unitigs = 0, singletons = 0, circular = 0;
    long long total_length = 0, longest_reads = 0, longest_length = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) out.utg_off[start_id[n_reads]] = start_off[n_reads];
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += stride) {
        const UtgPlace pl = place[r];
        out.index[r] = pl.y;
        if (pl.x < 0) { out.unitig[r] = -1; skipped += 1; continue; }
        const long long u = start_id[pl.x], base = start_off[pl.x];
        out.unitig[r] = (int32_t)u;
        out.order[base + pl.y] = (int32_t)r;
        if (pl.y == 0) {
            const long long length = ulen[r];
            const bool circ = cut && cut[r];
            out.utg_off[u] = base; out.utg_reads[u] = pl.z; out.utg_length[u] = length; out.utg_circular[u] = circ ? 1 : 0;
            unitigs += 1; singletons += pl.z == 1 ? 1u : 0u; circular += circ ? 1u : 0u;
            total_length += length;
            longest_reads = pl.z > longest_reads ? pl.z : longest_reads;
            longest_length = length > longest_length ? length : longest_length;
        }
    }
    // (all lanes are back together here)
    const unsigned counts[4] = {skipped, unitigs, singletons, circular};
    unsigned long long mine = wave_lane_totals(counts, lane);
    const long long tl = wave_reduce_add64(total_length), lr = utg_wave_max(longest_reads), ll = utg_wave_max(longest_length);
    if (lane == kUtgTotalLength) mine = (unsigned long long)tl;
    if (lane < kUtgLongestReads) { if (mine) atomicAdd(&ctl[kUtgCtlTotals + lane], mine); }
    else if (lane == kUtgLongestReads) { if (lr) atomicMax(&ctl[kUtgCtlTotals + lane], (unsigned long long)lr); }
    else if (lane == kUtgLongestLength) { if (ll) atomicMax(&ctl[kUtgCtlTotals + lane], (unsigned long long)ll); }
}

} // namespace raft
