// pipeline_plan.hpp -- the arithmetic of the chunked host pipeline (engine_pipeline.hip) as plain functions on host arrays: the
// sorted runs of a record stream, the chunk plan with its delta4 boundary moves, where every context's outputs start in the
// caller's arrays, and what the host derives from plain columns before they cross the link.  No HIP call and no HIP header:
// a host compiler alone builds it (tests/pipeline_plan_check.cpp does, under the sanitizers).
#pragma once
#include <algorithm>
#include <cstdint>
#include <functional>
#include <thread>
#include <vector>

namespace raft {

constexpr int kPlanSeg = 4;            // pieces a chunk keeps: raft_types.hpp kMaxSeg (engine_pipeline.hip asserts that they agree)

inline void host_parallel(int n_tasks, const std::function<void(int)> &fn)
{
    std::vector<std::thread> th;
    for (int t = 1; t < n_tasks; ++t) th.emplace_back([&fn, t] { fn(t); });
    if (n_tasks > 0) fn(0);
    for (auto &x : th) x.join();
}

// The one division by the window size: n / reso == (n * magic) >> shift for 0 <= n < 2^31, the multiply-high identity the
// kernels use (engine.hip run_pass, div_magic).
struct WindowDiv {
    uint64_t magic = 1;
    int shift = 0;
    explicit WindowDiv(int32_t reso)
    {
        int lg = 0;
        while ((1u << lg) < (uint32_t)reso) ++lg;
        if (reso > 1) { magic = (1ull << (31 + lg)) / (uint32_t)reso + 1ull; shift = 31 + lg; }
    }
    inline __attribute__((always_inline)) uint32_t index(uint32_t coord) const { return (uint32_t)(((uint64_t)coord * magic) >> shift); }
    // ceil(len / reso), exact for 0 <= len < 2^31 (a negative length has no windows: count_windows reports it)
    inline __attribute__((always_inline)) long long windows(int32_t len) const { return len > 0 ? (long long)index((uint32_t)len - 1u) + 1 : 0; }
};

// windows of n reads: sum ceil(len / reso); -1 when a length is negative (the pass reports it)
inline long long count_windows(const int32_t *len, long long n, const WindowDiv &div)
{
    long long w = 0;
    int32_t any_neg = 0;
    for (long long i = 0; i < n; ++i) {
        any_neg |= len[i];
        w += div.windows(len[i]);
    }
    return any_neg < 0 ? -1 : w;
}

// Sorted runs of the record stream from 8 k samples + bisection; -1 when there are more than kPlanSeg.
inline int guess_segments(const int32_t *q, long long n, long long (&start)[kPlanSeg + 1])
{
    const long long S = std::min<long long>(n, 8192);
    int n_seg = 1;
    start[0] = 0;
    long long prev_pos = 0;
    for (long long i = 1; i < S; ++i) {
        const long long pos = i * (n - 1) / (S - 1);
        if (q[pos] < q[prev_pos]) {                  // a run ends in (prev_pos, pos]: first position below q[prev_pos]
            long long lo = prev_pos, hi = pos;
            const int32_t v = q[prev_pos];
            while (hi - lo > 1) {
                const long long mid = lo + (hi - lo) / 2;
                if (q[mid] >= v) lo = mid; else hi = mid;
            }
            if (n_seg == kPlanSeg) return -1;
            start[n_seg++] = hi;
        }
        prev_pos = pos;
    }
    start[n_seg] = n;
    return n_seg;
}

inline long long lower_bound_ids(const int32_t *q, long long lo, long long hi, int32_t r)   // first position in [lo, hi) with q >= r
{
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        if (q[mid] < r) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// an explicit n_chunks is honoured from tiny inputs on (that is how the tests reach every shape of the plan); left to the
// engine, a job is cut from ~200 MB up: below that one piece is as fast
inline bool big_enough(long long n_rec, long long n_reads, int n_chunks)
{
    return n_chunks > 0 ? (n_rec >= 2 && n_reads >= 2) : (n_rec >= (1 << 24) && n_reads >= 4096);
}

inline long long default_chunks(long long n_rec, long long n_reads, int n_ctx)
{
    return std::min<long long>(std::min<long long>(32LL * n_ctx, std::max<long long>(2LL * n_ctx, n_rec / (24LL << 20))), n_reads / 1024);
}

// A host-to-host job's input in one of its three forms: plain columns (query ids per record), grouped (n_runs, rec_offset: the
// caller's per-read record offsets instead of the query column) and window records (grouped, one word per record instead of
// qs / qe).
struct HostInput {
    int32_t n_reads = 0;
    const int32_t *read_len = nullptr;
    int64_t n_rec = 0;
    const int32_t *qid = nullptr, *qs = nullptr, *qe = nullptr, *tid = nullptr, *ts = nullptr, *te = nullptr;
    int32_t n_runs = 0;
    const int64_t *rec_offset = nullptr;
    const uint32_t *win = nullptr;
    enum Form { kColumns, kGrouped, kWindows };
    Form form() const { return win ? kWindows : (rec_offset ? kGrouped : kColumns); }
    long long off_at(int g, long long r) const { return rec_offset[(long long)g * ((long long)n_reads + 1) + r]; }
};

struct Piece { long long lo, hi; };

struct ChunkPlan {
    int32_t r0, r1;
    Piece piece[kPlanSeg];
    long long n_rec;
    long long win_lo;            // delta4: windows of the reads before r0 (where the chunk's coverage begins in the caller's array)
};

// Read boundaries that balance the records, then one piece per run and chunk.  seg[0 .. n_seg]: the sorted runs of the stream.
// An empty plan: a read length is negative (met while counting windows for delta4; the one-piece pass reports it).
inline std::vector<ChunkPlan> plan_chunks(const HostInput &in, const long long *seg, int n_seg, int want, bool ramp, bool d4, int32_t reso)
{
    const bool grouped = in.form() != HostInput::kColumns;
    const int32_t n_reads = in.n_reads;
    const long long n_rec = in.n_rec;
    auto first_of = [&](int g, long long lo, int32_t r) {   // first record of read r in run g, at or after lo
        if (!grouped) return lower_bound_ids(in.qid, lo, seg[g + 1], r);
        return std::min(std::max(in.off_at(g, r), lo), seg[g + 1]);   // (offsets that step back: the device reports them)
    };
    auto below = [&](int32_t r) {                // records with a query id < r (if the runs are sorted)
        long long n = 0;
        for (int k = 0; k < n_seg; ++k) n += first_of(k, seg[k], r) - seg[k];
        return n;
    };
    std::vector<int32_t> bound{0};
    for (int k = 1; k < want; ++k) {
        // (ramp: the first and the last chunk are half the others' size)
        const long long target = ramp ? (long long)((double)n_rec * (k - 0.5) / (want - 1.0)) : n_rec * k / want;
        int32_t lo = bound.back(), hi = n_reads;
        while (lo < hi) {
            const int32_t mid = lo + (hi - lo) / 2;
            if (below(mid) < target) lo = mid + 1; else hi = mid;
        }
        if (lo > bound.back() && lo < n_reads) bound.push_back(lo);
    }
    bound.push_back(n_reads);
    std::vector<long long> win_before;           // delta4: windows before every boundary
    if (d4) {
        // delta4: a chunk's windows must begin on a multiple of 4 (its nibbles fill whole ushorts of the caller's array;
        // the anchors' blocks may begin anywhere, see PileupArgs::d4_shift): every inner boundary moves forward to the
        // next read that does -- a few reads on.  The windows before the boundaries are counted by one thread per chunk.
        const WindowDiv div(reso);
        const size_t nb = bound.size() - 1;
        std::vector<long long> wsum(nb, 0);
        host_parallel((int)nb, [&](int k) { wsum[(size_t)k] = count_windows(in.read_len + bound[(size_t)k], bound[(size_t)k + 1] - bound[(size_t)k], div); });
        std::vector<int32_t> moved{0};
        win_before.push_back(0);
        long long before = 0;                       // windows before the ORIGINAL boundary k
        bool ok = true;
        for (size_t k = 1; k < nb && ok; ++k) {
            ok = wsum[k - 1] >= 0;
            before += wsum[k - 1];
            int32_t r = bound[k];
            long long w = before;
            if (r <= moved.back()) continue;        // (an earlier boundary moved past this one: dropped)
            while (ok && (w & 3) != 0 && r < n_reads) {
                const long long one = count_windows(in.read_len + r, 1, div);
                if (one < 0) ok = false;
                w += one; ++r;
            }
            if (ok && r < n_reads && (w & 3) == 0) {
                // (boundaries after this one still count from their ORIGINAL place: `before` is not touched)
                moved.push_back(r); win_before.push_back(w);
            }
        }
        if (!ok || wsum[nb - 1] < 0) return {};
        moved.push_back(n_reads);
        bound.swap(moved);
    }
    std::vector<ChunkPlan> plan;
    std::vector<long long> cur(seg, seg + n_seg);
    for (size_t k = 0; k + 1 < bound.size(); ++k) {
        ChunkPlan cp{};
        cp.r0 = bound[k]; cp.r1 = bound[k + 1]; cp.n_rec = 0;
        cp.win_lo = d4 ? win_before[k] : 0;
        for (int g = 0; g < n_seg; ++g) {
            const long long hi = (k + 2 == bound.size()) ? seg[g + 1] : first_of(g, cur[g], cp.r1);
            cp.piece[g] = Piece{cur[g], hi};
            cp.n_rec += hi - cur[g];
            cur[g] = hi;
        }
        plan.push_back(cp);
    }
    return plan;
}

// Where each context's outputs start in the caller's arrays: consecutive chunks each (the plan balances records per chunk).
// Windows are exact (sum of ceil(len / reso) over the reads before); repeats and fragments start at the bounds of raft_hip.h
// and are moved down when all contexts are done.  One context needs none of this: its rooms are the caller's capacities.
struct JobPlace {
    int first_chunk = 0, n_chunks = 0;
    long long bins0 = 0, rep0 = 0, frag0 = 0;
    long long rep_room = 0, frag_room = 0;
};
struct PlaceCaps { long long bins = 0, rep = 0, frag = 0; };     // what the caller's arrays must hold (several contexts)

// An empty result: a read length is negative (reported as RAFT_HIP_ERR_PARAM with its index by the one-piece pass).
inline std::vector<JobPlace> place_jobs(const std::vector<ChunkPlan> &plan, int n_job, const int32_t *read_len, long long minbins, long long interval_length,
                                        const WindowDiv &div, PlaceCaps *caps)
{
    const int n_ch = (int)plan.size();
    std::vector<JobPlace> jobs((size_t)n_job);
    PlaceCaps tot;
    int r = 0;
    for (int d = 0; d < n_job; ++d) {
        JobPlace &J = jobs[(size_t)d];
        J.first_chunk = n_ch * d / n_job; J.n_chunks = n_ch * (d + 1) / n_job - J.first_chunk;
        J.bins0 = tot.bins; J.rep0 = tot.rep; J.frag0 = tot.frag;
        if (n_job == 1) break;
        const int r_end = plan[(size_t)(J.first_chunk + J.n_chunks - 1)].r1;
        long long jb = 0, jl = 0;
        for (; r < r_end; ++r) {
            if (read_len[r] < 0) return {};
            jb += div.windows(read_len[r]); jl += read_len[r];
        }
        const long long n_r = r_end - plan[(size_t)J.first_chunk].r0;
        // sum floor(x_i / m) <= floor(sum x_i / m): the per-read bounds of raft_hip.h, summed, are at least these
        J.rep_room = (jb + n_r) / (minbins + 1); J.frag_room = jl / interval_length + 2 * n_r;
        tot.bins += jb; tot.rep += J.rep_room; tot.frag += J.frag_room;
    }
    *caps = tot;
    return jobs;
}

// What the engine's host side derives from the plain columns of a symmetric, sorted stream before they cross the link (SURVEY.md
// §8(d): the clock of a host-to-host job starts at the int32 columns): per piece of a chunk -- records [lo, hi) of one sorted run,
// reads [r0, r1) -- where every read's records begin (the grouped form of raft_hip_run_device_grouped) and the records as
// window records (one word: first window | one past the last << 16; repeat.hpp:69-72 uses nothing else of an interval).  4 bytes
// per record go up instead of 12, and the pass needs no look at the stream.  The ids are checked on the way (inside the
// chunk's reads, never stepping back): anything else, a negative coordinate or a window beyond 16 bits sends the job to the
// one-piece pass over the columns, which reports or handles it.  T threads share the piece.
// (Two loops, the first branch-free so that the compiler vectorises it: the window indices by multiply-high -- WindowDiv; a
// hardware division per coordinate made the derivation compute-bound at 10 cycles per record -- with the error conditions
// collected, not branched on; then the id column for the places where the read changes.)
static inline __attribute__((always_inline)) bool derive_body(int t, int T, const int32_t *qid, const int32_t *qs, const int32_t *qe, long long lo, long long hi,
                                                              int32_t r0, int32_t r1, const WindowDiv div, long long at, long long *off, uint32_t *win)
{
    const long long n = hi - lo;
    const int32_t nr = r1 - r0;
    if (n <= 0) { if (t == 0) for (int32_t j = 0; j <= nr; ++j) off[j] = at; return true; }
    const long long a = lo + n * t / T, b = lo + n * (t + 1) / T;
    if (a >= b) return true;
    {
        const int32_t *ps = qs + a, *pe = qe + a;
        uint32_t *pw = win + (a - lo);
        const long long cnt = b - a;
        uint32_t neg = 0, far = 0;
        for (long long i = 0; i < cnt; ++i) {
            const int32_t s0 = ps[i], e0 = pe[i];
            neg |= (uint32_t)(s0 | e0);
            const uint32_t first = div.index((uint32_t)s0);
            const uint32_t em = (uint32_t)(e0 > 0 ? e0 - 1 : 0);
            const uint32_t last1 = e0 > 0 ? div.index(em) + 1u : 0u;
            const uint32_t w = last1 > first ? (first | (last1 << 16)) : 0u;
            far |= last1 > first ? last1 : 0u;
            pw[i] = w;
        }
        if ((neg >> 31) || (far >> 16)) return false;      // a negative coordinate; a window index beyond 16 bits
    }
    int32_t prev = a == lo ? r0 - 1 : qid[a - 1];
    if (prev < r0 - 1 || prev >= r1) return false;
    for (long long i = a; i < b; ++i) {
        const int32_t q = qid[i];
        if (q != prev) {
            if (q < prev || q >= r1) return false;
            for (int32_t r = prev + 1; r <= q; ++r) off[r - r0] = at + (i - lo);      // (reads without records begin where the next one does)
            prev = q;
        }
    }
    if (b == hi) for (int32_t r = prev + 1; r <= r1; ++r) off[r - r0] = at + n;           // closing entries
    return true;
}
#if defined(__x86_64__)
__attribute__((target("avx2"))) static bool derive_slice_avx2(int t, int T, const int32_t *qid, const int32_t *qs, const int32_t *qe, long long lo, long long hi,
                                                              int32_t r0, int32_t r1, const WindowDiv &div, long long at, long long *off, uint32_t *win)
{
    return derive_body(t, T, qid, qs, qe, lo, hi, r0, r1, div, at, off, win);
}
#endif
static inline bool derive_slice(int t, int T, const int32_t *qid, const int32_t *qs, const int32_t *qe, long long lo, long long hi, int32_t r0, int32_t r1,
                                const WindowDiv &div, long long at, long long *off, uint32_t *win)
{
#if defined(__x86_64__)
    static const bool avx2 = __builtin_cpu_supports("avx2");
    if (avx2) return derive_slice_avx2(t, T, qid, qs, qe, lo, hi, r0, r1, div, at, off, win);
#endif
    return derive_body(t, T, qid, qs, qe, lo, hi, r0, r1, div, at, off, win);
}

} // namespace raft
