// frag_ovl.hpp -- the record stream against the fragment table (raft_hip_frag_overlaps_device / _host, include/raft_hip_frag.h): per
// fragment the overlap sides that touch it, span it end to end, and span it with the partner's side still inside one fragment of the
// partner (contained); its bases inside the read's repeats; per read its contained fragments.
//
// Four kernels and the scan between them:
//   frag_digest_kernel  a lane per read: checks the read's slice of frag_offset and its rows (0 <= fb <= fe, neither bound descends) and
//                       writes 16 bytes per read (FragDigest): where its rows begin, how many there are and
//                           n == 1   the one row [x, y) itself -- the common case: a side is answered from this gather alone
//                           n >  1   the hull [x, y) = [fb of the first row, fe of the last]: a side outside it touches nothing,
//                                    one inside goes to the CSR arrays with binary searches
//   frag_side_kernel    a streaming kernel of record_stream.hpp's shape.  fb and fe do not descend within a read, so each property
//                       selects a contiguous range of rows, a suffix cut with a prefix:
//                           touched    [lt, ht)   lt = first row with fe > a, ht = first row at or behind lt with fb >= b
//                           spanned    [ls, hs)   inside [lt, ht): ls = first row with fb >= a, hs = first row behind with fe > b
//                           contained  [ls, hs)   when the partner is whole: the last row g of the partner with fb[g] <= c has d <= fe[g]
//                       (two searches over the read's rows, two over the touched range -- a handful of rows --, one over the partner's).
//                       The counts are difference arrays over the n_frag + 1 row slots, +1 at a range's first row and -1 behind its last,
//                       packed 16 bytes a slot (FragSlot): touch and span share one 64-bit word, so the four ends of a side's two ranges cost
//                       two to four 64-bit atomic adds on one or two neighbouring lines, and the contained range two more on the same slots.
//   scan                device_scan.hpp's two kernels over the three sums at once; the apply kernel's hook writes the inclusive sums as
//                       the int32 counts (FragCounts).  A -1 that lands on the next read's first slot is what ends the range there.
//   frag_reads_kernel   a lane per read over its rows: the row's bases inside the set union of the read's repeat runs (ovl_class.hpp's
//                       digest and sweep), the read's contained rows, the totals.
// The record kernel and the reads kernel look at ctl[kFragBadTable] first and leave when the digest kernel found the table broken: they
// would read out of bounds.  No kernel waits for another workgroup; every loop is bounded by a read's row count or its run count.
#pragma once
#include "raft_types.hpp"
#include "wave.hpp"
#include "record_stream.hpp"
#include "census.hpp"
#include "ovl_class.hpp"
#include "device_scan.hpp"

namespace raft {

// control words (unsigned long long each)
constexpr int kFragFirstBad = 0;         // smallest record index with an id out of range; ~0 = none
constexpr int kFragBadTable = 1;         // != 0: the fragment table is not what the header asks for
constexpr int kFragBadRepeats = 2;       // != 0: rep_offset is not (ovl_digest_kernel's verdict: it is handed ctl + 1)
constexpr int kFragTotals = 3;           // untouched, spanned, contained, contained with repeat; reads whole spanned, any, all contained
constexpr int kFragCtlWords = 10;
static_assert(kFragBadRepeats - 1 == kOvlBadOffsets, "ovl_digest_kernel writes its verdict to the word behind the pointer it is given");

struct FragDigest { int32_t k0, n, x, y; };
// a row slot of the difference arrays: ts = touch + (span << 32) as ONE 64-bit sum of the sign-extended steps (the low half borrows
// from the high half while the touch sum is negative: frag_slot_sums undoes it), c = contained
struct FragSlot { unsigned long long ts, c; };

__device__ __forceinline__ void frag_slot_sums(const FragSlot s, long long (&v)[3])
{
    const int32_t t = (int32_t)(unsigned)s.ts;
    v[0] = t;
    v[1] = (int32_t)(unsigned)(s.ts >> 32) + (t < 0 ? 1 : 0);
    v[2] = (int32_t)(unsigned)s.c;
}

__global__ __launch_bounds__(256) void frag_digest_kernel(const long long *__restrict__ off, const int32_t *__restrict__ fb, const int32_t *__restrict__ fe,
                                                          int32_t n_reads, long long n_frag, FragDigest *__restrict__ digest,
                                                          unsigned long long *__restrict__ ctl)
{
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_reads) return;
    if (r == n_reads) {                                      // the one lane behind the reads: the two ends
        if (off[0] != 0 || off[n_reads] != n_frag) atomicOr(&ctl[kFragBadTable], 1ull);
        return;
    }
    const long long k0 = off[r], k1 = off[r + 1];
    FragDigest d{0, 0, 0, 0};
    if (k0 < 0 || k1 < k0 || k1 > n_frag) {
        atomicOr(&ctl[kFragBadTable], 1ull);
    } else if (k1 > k0) {
        int32_t pb = 0, pe = 0;                              // (the bounds of the row before; 0: no bound is negative)
        bool bad = false;
        for (long long k = k0; k < k1; ++k) {
            const int32_t b = fb[k], e = fe[k];
            bad = bad || b < pb || e < pe || e < b;
            pb = b; pe = e;
        }
        if (bad) atomicOr(&ctl[kFragBadTable], 1ull);
        d = FragDigest{(int32_t)k0, (int32_t)(k1 - k0), fb[k0], pe};
    }
    digest[r] = d;
}

struct FragArgs {
    const int32_t *len, *qid, *qs, *qe, *tid, *ts, *te;
    long long n_rec;
    int32_t n_reads, symmetric;
    const int32_t *fb, *fe;
    const FragDigest *digest;
    FragSlot *slot;                                          // [n_frag + 1], zeroed before the launch
    unsigned *whole;                                         // [n_reads], zeroed before the launch: bit 0 = a counted side spans the read
    unsigned long long *ctl;
};

// first row in [lo, hi) of the read whose rows begin at v with v[k] > x (kStrict) / v[k] >= x; hi when there is none
template <bool kStrict>
__device__ __forceinline__ int frag_first(const int32_t *__restrict__ v, int lo, int hi, int x)
{
    while (lo < hi) {                                        // (halves the range: at most 31 turns)
        const int m = lo + ((hi - lo) >> 1);
        const int w = v[m];
        if (kStrict ? w > x : w >= x) hi = m; else lo = m + 1;
    }
    return lo;
}

// is [c, d) inside one row of the read with digest p?  fb and fe do not descend: of the rows with fb <= c the last has the largest fe
__device__ __forceinline__ bool frag_partner_whole(const FragArgs &A, const FragDigest p, int c, int d)
{
    if (d <= c || p.n == 0 || c < p.x || d > p.y) return false;
    if (p.n == 1) return true;
    const int m = frag_first<true>(A.fb + p.k0, 0, p.n, c);
    return m > 0 && A.fe[p.k0 + m - 1] >= d;
}

__device__ __forceinline__ void frag_add(unsigned long long *word, long long step)
{
    atomicAdd(word, (unsigned long long)step);
}

// One counted side [a, b) on the read with digest r, its partner side [c, d) on the read with digest p.
__device__ __forceinline__ void frag_side(const FragArgs &A, const FragDigest r, int a, int b, const FragDigest p, int c, int d)
{
    if (b <= a || r.n == 0 || r.y <= a || r.x >= b) return;  // (outside the hull: no row has fe > a and fb < b)
    int lt = 0, ht = 1, ls, hs = 1;
    if (r.n == 1) ls = (r.x >= a && r.y <= b) ? 0 : 1;
    else {
        const int32_t *fb = A.fb + r.k0, *fe = A.fe + r.k0;
        lt = frag_first<true>(fe, 0, r.n, a);
        ht = frag_first<false>(fb, lt, r.n, b);
        if (ht <= lt) return;
        ls = frag_first<false>(fb, lt, ht, a);
        hs = frag_first<true>(fe, ls, ht, b);
    }
    FragSlot *s = A.slot + r.k0;
    constexpr long long kSpan = 1ll << 32;
    if (hs <= ls) {                                          // touched, none spanned
        frag_add(&s[lt].ts, 1); frag_add(&s[ht].ts, -1);
        return;
    }
    if (ls == lt) frag_add(&s[lt].ts, 1 + kSpan);
    else { frag_add(&s[lt].ts, 1); frag_add(&s[ls].ts, kSpan); }
    if (hs == ht) frag_add(&s[ht].ts, -1 - kSpan);
    else { frag_add(&s[hs].ts, -kSpan); frag_add(&s[ht].ts, -1); }
    if (frag_partner_whole(A, p, c, d)) { frag_add(&s[ls].c, 1); frag_add(&s[hs].c, -1); }
}

template <bool kVec>
__global__ __launch_bounds__(kStreamThreads) void frag_side_kernel(FragArgs A)
{
    constexpr int R = kStreamLaneRecords;
    if (A.ctl[kFragBadTable]) return;                        // (uniform: the digest kernel's verdict, written before this launch)
    const int lane = (int)threadIdx.x & (kWave - 1);
    const unsigned n_reads = (unsigned)A.n_reads;
    stream_for_each_group(A.n_rec, lane, [&](const long long first) {
        LaneRecords r;
        stream_load_records<kVec>(A.qid, A.qs, A.qe, A.tid, A.ts, A.te, first, A.n_rec, true, r);
        // the gathers of the lane's eight sides first, all in flight together
        FragDigest dq[R], dt[R];
        bool ok[R];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const IdsValid v = stream_check_ids(first + i < A.n_rec, first + i, r.q[i], r.t[i], n_reads, &A.ctl[kFragFirstBad]);
            ok[i] = v.q && v.t && r.q[i] != r.t[i];          // (a record of a read with itself contributes nothing)
            dq[i] = dt[i] = FragDigest{0, 0, 0, 0};
            if (ok[i]) {
                dq[i] = A.digest[r.q[i]];
                dt[i] = A.digest[r.t[i]];
            }
        }
#pragma unroll
        for (int i = 0; i < R; ++i) {
            if (!ok[i]) continue;
            frag_side(A, dq[i], r.qs[i], r.qe[i], dt[i], r.ts[i], r.te[i]);
            // the rule before fragmentation looks at the start before it gathers the length
            if (r.qs[i] <= 0 && r.qe[i] > r.qs[i] && r.qe[i] >= A.len[r.q[i]]) ovl_flag(&A.whole[r.q[i]], 1u);
            if (!A.symmetric) {
                frag_side(A, dt[i], r.ts[i], r.te[i], dq[i], r.qs[i], r.qe[i]);
                if (r.ts[i] <= 0 && r.te[i] > r.ts[i] && r.te[i] >= A.len[r.t[i]]) ovl_flag(&A.whole[r.t[i]], 1u);
            }
        }
    });
}

// device_scan.hpp's loader and hook: the three sums of a slot in; the inclusive sums -- the counts of row i -- out
struct FragLoader {
    const FragSlot *slot;
    __device__ void operator()(long long i, long long (&v)[3]) const { frag_slot_sums(slot[i], v); }
};
struct FragCounts {
    int32_t *touch, *span, *cont;
    template <int K> __device__ void operator()(long long i, const long long (&first)[K], const long long (&v)[K]) const
    {
        touch[i] = (int32_t)(first[0] + v[0]); span[i] = (int32_t)(first[1] + v[1]); cont[i] = (int32_t)(first[2] + v[2]);
    }
    template <int K> __device__ void closing(const long long (&)[K]) const {}
};

// |[a, b) intersected with U(r)|: ovl_side's two cases (ovl_class.hpp) without the classes -- the one piece of the digest, or the sweep
// over the runs in ascending rep_s with a covered-to position when the row reaches into the hull of several
__device__ __forceinline__ int32_t frag_repeat_bases(const long long *__restrict__ rep_off, const int32_t *__restrict__ rep_s, const int32_t *__restrict__ rep_e,
                                                     const OvlDigest d, long long r, int a, int b)
{
    if (b <= a) return 0;
    if (d.x <= d.y) {
        const int lo = a > d.x ? a : d.x, hi = b < d.y ? b : d.y;
        return hi > lo ? hi - lo : 0;
    }
    if ((b < d.x ? b : d.x) <= (a > d.y ? a : d.y)) return 0;
    const long long k1 = rep_off[r + 1];
    long long rep = 0;
    int cur = a;
    for (long long k = rep_off[r]; k < k1; ++k) {
        const int s = rep_s[k];
        if (s >= b) break;
        const int e = rep_e[k];
        const int lo = s > cur ? s : cur, hi = e < b ? e : b;
        if (hi > lo) { rep += (long long)hi - lo; cur = hi; }
    }
    return (int32_t)rep;                                     // (at most b - a, and 0 <= a)
}

struct FragReadsArgs {
    const long long *off;
    const int32_t *fb, *fe;
    int32_t n_reads;
    const int32_t *touch, *span, *cont;
    const long long *rep_off;                                // NULL: no annotation, frag_repeat is 0
    const int32_t *rep_s, *rep_e;
    const OvlDigest *rep_digest;
    const unsigned *whole;
    int32_t *frag_repeat, *read_contained;
    unsigned long long *ctl;
};

__global__ __launch_bounds__(256) void frag_reads_kernel(FragReadsArgs A)
{
    if (A.ctl[kFragBadTable] | A.ctl[kFragBadRepeats]) return;
    const long long stride = (long long)gridDim.x * blockDim.x;
    unsigned tot[7] = {0, 0, 0, 0, 0, 0, 0};
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < A.n_reads; r += stride) {
        const long long k0 = A.off[r], k1 = A.off[r + 1];
        const OvlDigest d = A.rep_off ? A.rep_digest[r] : OvlDigest{0, 0};
        int contained = 0;
        for (long long k = k0; k < k1; ++k) {
            const int32_t rep = A.rep_off ? frag_repeat_bases(A.rep_off, A.rep_s, A.rep_e, d, r, A.fb[k], A.fe[k]) : 0;
            A.frag_repeat[k] = rep;
            const bool c = A.cont[k] > 0;
            tot[0] += A.touch[k] == 0 ? 1 : 0; tot[1] += A.span[k] > 0 ? 1 : 0; tot[2] += c ? 1 : 0; tot[3] += c && rep > 0 ? 1 : 0;
            contained += c ? 1 : 0;
        }
        A.read_contained[r] = contained;
        tot[4] += A.whole[r] & 1u; tot[5] += contained > 0 ? 1 : 0; tot[6] += (contained > 0 && contained == k1 - k0) ? 1 : 0;
    }
    // (all lanes are back together here)
    wave_flush_totals(tot, &A.ctl[kFragTotals], (int)threadIdx.x & (kWave - 1));
}

} // namespace raft
