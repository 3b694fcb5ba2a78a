// pipeline_plan_check.cpp -- raft_amd/csrc/pipeline_plan.hpp on its own: the window division, the sorted runs, the chunk plan, the
// placement of the contexts' outputs and the derivation of window records, on small inputs made here.  No HIP: a host compiler
// builds it (tests/test_pipeline_plan.py: under the address and undefined-behaviour sanitizers).  `--print` writes the plans of
// the six literal cases in the form they are kept in below.
#include "../raft_amd/csrc/pipeline_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace raft;

static int g_failed = 0;
#define CHECK(cond, ...)                                                                   \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            if (++g_failed <= 20) { fprintf(stderr, "%s:%d: %s -- ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } \
        }                                                                                  \
    } while (0)

// ---- synthetic streams: n_seg runs sorted by query id, as plain columns and as grouped offsets
enum Shape { kEven, kGaps, kOneRead };
struct Stream {
    int32_t n_reads = 0;
    int n_seg = 0;
    std::vector<int32_t> len, qid, qs, qe;
    std::vector<int64_t> off;                     // n_seg rows of n_reads + 1 absolute positions
    long long seg[kPlanSeg + 1] = {};
    HostInput columns() const
    {
        HostInput in;
        in.n_reads = n_reads; in.read_len = len.data(); in.n_rec = (int64_t)qid.size();
        in.qid = qid.data(); in.qs = qs.data(); in.qe = qe.data();
        return in;
    }
    HostInput grouped() const
    {
        HostInput in = columns();
        in.qid = nullptr; in.n_runs = n_seg; in.rec_offset = off.data();
        return in;
    }
};

static Stream make_stream(int32_t n_reads, int n_seg, Shape shape, int32_t reso = 50)
{
    Stream s;
    s.n_reads = n_reads; s.n_seg = n_seg;
    uint32_t x = 12345u + (uint32_t)n_reads * 31u + (uint32_t)n_seg;
    for (int32_t r = 0; r < n_reads; ++r) { x = x * 1664525u + 1013904223u; s.len.push_back(100 + (int32_t)((x >> 12) % 30000u)); }
    s.off.assign((size_t)n_seg * ((size_t)n_reads + 1), 0);
    for (int g = 0; g < n_seg; ++g) {
        s.seg[g] = (long long)s.qid.size();
        for (int32_t r = 0; r < n_reads; ++r) {
            s.off[(size_t)g * ((size_t)n_reads + 1) + (size_t)r] = (int64_t)s.qid.size();
            int n = (r * 7 + g * 3) % 5;
            if (shape == kGaps && r % 3 != 1) n = 0;
            if (shape == kOneRead) n = r == n_reads / 2 ? 9 : 0;
            for (int j = 0; j < n; ++j) {
                const int32_t a = (int32_t)(((long long)s.len[(size_t)r] * j) / (n + 1));
                s.qid.push_back(r); s.qs.push_back(a); s.qe.push_back(std::min(s.len[(size_t)r], a + 3 * reso + j));
            }
        }
        s.off[(size_t)g * ((size_t)n_reads + 1) + (size_t)n_reads] = (int64_t)s.qid.size();
    }
    s.seg[n_seg] = (long long)s.qid.size();
    return s;
}

// ---- WindowDiv against plain division
static void check_window_div()
{
    for (int32_t reso : {1, 2, 50, 1000, 32767}) {
        const WindowDiv div(reso);
        const long long lens[] = {0, 1, reso - 1, reso, reso + 1, 65535LL * reso, 2147483647LL};
        for (long long len : lens) {
            if (len > 2147483647LL) continue;
            CHECK(div.windows((int32_t)len) == (len + reso - 1) / reso, "reso %d len %lld: %lld", reso, len, div.windows((int32_t)len));
            CHECK(div.index((uint32_t)len) == (uint32_t)(len / reso), "reso %d x %lld: %u", reso, len, div.index((uint32_t)len));
        }
        const int32_t three[3] = {reso, 2 * reso + 1, 0};
        CHECK(count_windows(three, 3, div) == 4, "reso %d", reso);
        const int32_t neg[3] = {reso, -1, 7};
        CHECK(count_windows(neg, 3, div) == -1, "reso %d", reso);
        CHECK(count_windows(neg, 0, div) == 0, "reso %d", reso);
    }
}

// ---- guess_segments
static void check_guess_segments()
{
    for (int n_seg : {1, 2, 4, 5}) {
        std::vector<int32_t> q;
        std::vector<long long> want{0};
        for (int g = 0; g < n_seg; ++g) {
            const int n = g == 1 ? 1 : 300 + 17 * g;            // (the second run: one record, between a higher and a lower id)
            for (int i = 0; i < n; ++i) q.push_back(g == 1 ? 1 : i / 2);
            want.push_back((long long)q.size());
        }
        long long start[kPlanSeg + 1];
        const int got = guess_segments(q.data(), (long long)q.size(), start);
        if (n_seg == 5) { CHECK(got == -1, "five runs: %d", got); continue; }
        CHECK(got == n_seg, "%d runs: %d", n_seg, got);
        for (int g = 0; g <= n_seg && got == n_seg; ++g) CHECK(start[g] == want[(size_t)g], "%d runs, start[%d] = %lld", n_seg, g, start[g]);
    }
    const int32_t one[1] = {3};
    long long start[kPlanSeg + 1];
    CHECK(guess_segments(one, 1, start) == 1 && start[0] == 0 && start[1] == 1, "a stream of one record");
}

// ---- plan_chunks: the invariants of every plan
static void check_plan(const char *what, const Stream &s, const HostInput &in, const std::vector<ChunkPlan> &plan, bool d4, int32_t reso)
{
    CHECK(!plan.empty(), "%s: no plan", what);
    if (plan.empty()) return;
    CHECK(plan.front().r0 == 0 && plan.back().r1 == s.n_reads, "%s: ends %d %d", what, plan.front().r0, plan.back().r1);
    long long total = 0;
    std::vector<long long> cur(s.seg, s.seg + s.n_seg);
    const WindowDiv div(reso);
    for (size_t k = 0; k < plan.size(); ++k) {
        const ChunkPlan &cp = plan[k];
        CHECK(cp.r0 < cp.r1, "%s: chunk %zu [%d, %d)", what, k, cp.r0, cp.r1);
        if (k) CHECK(cp.r0 == plan[k - 1].r1, "%s: chunk %zu begins at %d", what, k, cp.r0);
        long long n = 0;
        for (int g = 0; g < s.n_seg; ++g) {
            CHECK(cp.piece[g].lo == cur[(size_t)g] && cp.piece[g].hi >= cp.piece[g].lo, "%s: chunk %zu run %d [%lld, %lld)", what, k, g, cp.piece[g].lo, cp.piece[g].hi);
            for (long long i = cp.piece[g].lo; i < cp.piece[g].hi; ++i)
                CHECK(s.qid[(size_t)i] >= cp.r0 && s.qid[(size_t)i] < cp.r1, "%s: chunk %zu record %lld of read %d", what, k, i, s.qid[(size_t)i]);
            cur[(size_t)g] = cp.piece[g].hi;
            n += cp.piece[g].hi - cp.piece[g].lo;
        }
        CHECK(n == cp.n_rec, "%s: chunk %zu n_rec %lld", what, k, cp.n_rec);
        total += cp.n_rec;
        if (d4) CHECK((cp.win_lo & 3) == 0 && cp.win_lo == count_windows(in.read_len, cp.r0, div), "%s: chunk %zu win_lo %lld", what, k, cp.win_lo);
        else CHECK(cp.win_lo == 0, "%s: chunk %zu win_lo %lld", what, k, cp.win_lo);
    }
    for (int g = 0; g < s.n_seg; ++g) CHECK(cur[(size_t)g] == s.seg[g + 1], "%s: run %d ends at %lld", what, g, cur[(size_t)g]);
    CHECK(total == in.n_rec, "%s: %lld records", what, total);
}

static void check_plan_invariants()
{
    const int32_t reso = 50;
    for (int32_t n_reads : {2, 5, 1000})
        for (int n_seg : {1, 2, 4})
            for (Shape shape : {kEven, kGaps, kOneRead}) {
                const Stream s = make_stream(n_reads, n_seg, shape, reso);
                for (int want : {2, 5, 23, (int)n_reads})
                    for (int form = 0; form < 2; ++form)
                        for (int d4 = 0; d4 < 2; ++d4) {
                            const HostInput in = form ? s.grouped() : s.columns();
                            char what[128];
                            snprintf(what, sizeof what, "reads %d runs %d shape %d want %d form %d d4 %d", n_reads, n_seg, (int)shape, want, form, d4);
                            const int w = std::min(want, (int)n_reads);
                            if (d4 && w > 23 && (shape != kEven || form)) continue;   // (delta4 counts windows with a thread per chunk: a thousand once)
                            check_plan(what, s, in, plan_chunks(in, s.seg, n_seg, w, false, d4 != 0, reso), d4 != 0, reso);
                            if (w >= 6) check_plan(what, s, in, plan_chunks(in, s.seg, n_seg, w, true, d4 != 0, reso), d4 != 0, reso);
                        }
            }
    // a negative read length is the planner's one failure (met only where windows are counted: delta4)
    Stream s = make_stream(1000, 2, kEven, reso);
    s.len[500] = -1;
    CHECK(plan_chunks(s.columns(), s.seg, 2, 5, false, true, reso).empty(), "negative length, delta4");
    CHECK(plan_chunks(s.columns(), s.seg, 2, 5, false, false, reso).size() == 5, "negative length, no delta4");
}

// delta4: boundaries that move.  One record per read, one boundary per read.
static void check_d4_moves()
{
    const int32_t reso = 50, n_reads = 12;
    Stream s = make_stream(n_reads, 1, kEven, reso);
    s.qid.clear(); s.qs.clear(); s.qe.clear();
    for (int32_t r = 0; r < n_reads; ++r) { s.qid.push_back(r); s.qs.push_back(0); s.qe.push_back(10); }
    s.seg[0] = 0; s.seg[1] = n_reads;
    // every read one window: boundary 1 moves to read 4 and passes the original boundaries 2, 3 (and meets 4): dropped
    for (int32_t r = 0; r < n_reads; ++r) s.len[(size_t)r] = reso;
    std::vector<ChunkPlan> plan = plan_chunks(s.columns(), s.seg, 1, n_reads, false, true, reso);
    check_plan("d4 dropped", s, s.columns(), plan, true, reso);
    CHECK(plan.size() == 3, "d4 dropped: %zu chunks", plan.size());
    for (size_t k = 0; k < plan.size() && plan.size() == 3; ++k)
        CHECK(plan[k].r0 == (int32_t)(4 * k) && plan[k].r1 == (int32_t)(4 * k + 4) && plan[k].win_lo == (long long)(4 * k), "d4 dropped: chunk %zu [%d, %d)", k, plan[k].r0, plan[k].r1);
    // one window, then four per read: no read begins on a multiple of 4 -- every boundary disappears
    for (int32_t r = 0; r < n_reads; ++r) s.len[(size_t)r] = r == 0 ? reso : 4 * reso;
    plan = plan_chunks(s.columns(), s.seg, 1, n_reads, false, true, reso);
    check_plan("d4 vanished", s, s.columns(), plan, true, reso);
    CHECK(plan.size() == 1, "d4 vanished: %zu chunks", plan.size());
}

// ---- place_jobs
static void check_place_jobs()
{
    const int32_t reso = 50;
    const long long minbins = 7, interval_length = 1000;
    const Stream s = make_stream(1000, 2, kEven, reso);
    const HostInput in = s.columns();
    const WindowDiv div(reso);
    const std::vector<ChunkPlan> plan = plan_chunks(in, s.seg, 2, 23, false, false, reso);
    for (int n_job : {1, 2, 3, 5}) {
        PlaceCaps caps;
        const std::vector<JobPlace> jobs = place_jobs(plan, n_job, in.read_len, minbins, interval_length, div, &caps);
        CHECK((int)jobs.size() == n_job, "%d jobs: %zu", n_job, jobs.size());
        if ((int)jobs.size() != n_job) continue;
        long long rep = 0, frag = 0;
        int next = 0;
        for (int d = 0; d < n_job; ++d) {
            const JobPlace &J = jobs[(size_t)d];
            CHECK(J.first_chunk == next && J.n_chunks >= 1, "%d jobs: job %d chunks %d + %d", n_job, d, J.first_chunk, J.n_chunks);
            next = J.first_chunk + J.n_chunks;
            if (n_job == 1) { CHECK(J.bins0 == 0 && J.rep0 == 0 && J.frag0 == 0 && J.rep_room == 0 && J.frag_room == 0, "one job"); continue; }
            const int32_t ra = plan[(size_t)J.first_chunk].r0, rb = plan[(size_t)(next - 1)].r1;
            long long before = 0, jb = 0, jl = 0;
            for (int32_t r = 0; r < ra; ++r) before += (s.len[(size_t)r] + reso - 1) / reso;
            for (int32_t r = ra; r < rb; ++r) { jb += (s.len[(size_t)r] + reso - 1) / reso; jl += s.len[(size_t)r]; }
            CHECK(J.bins0 == before, "%d jobs: job %d bins0 %lld", n_job, d, J.bins0);
            CHECK(J.rep0 == rep && J.frag0 == frag, "%d jobs: job %d rep0 %lld frag0 %lld", n_job, d, J.rep0, J.frag0);
            // raft_hip.h: repeats <= (windows + reads) / (minbins + 1), fragments <= bases / interval_length + 2 * reads
            CHECK(J.rep_room == (jb + (rb - ra)) / (minbins + 1), "%d jobs: job %d rep_room %lld", n_job, d, J.rep_room);
            CHECK(J.frag_room == jl / interval_length + 2 * (rb - ra), "%d jobs: job %d frag_room %lld", n_job, d, J.frag_room);
            rep += J.rep_room; frag += J.frag_room;
            if (d == n_job - 1) CHECK(caps.bins == before + jb, "%d jobs: bins %lld", n_job, caps.bins);
        }
        CHECK(next == (int)plan.size(), "%d jobs: %d chunks placed", n_job, next);
        CHECK(caps.rep == rep && caps.frag == frag, "%d jobs: caps %lld %lld", n_job, caps.rep, caps.frag);
    }
    Stream neg = make_stream(1000, 2, kEven, reso);
    neg.len[700] = -5;
    PlaceCaps caps;
    CHECK(place_jobs(plan, 2, neg.len.data(), minbins, interval_length, div, &caps).empty(), "negative length");
}

// ---- derive_slice against a per-record model
static void check_derive(const Stream &s, int32_t r0, int32_t r1, int32_t reso, int T)
{
    const long long lo = std::lower_bound(s.qid.begin(), s.qid.begin() + s.seg[1], r0) - s.qid.begin();
    const long long hi = std::lower_bound(s.qid.begin(), s.qid.begin() + s.seg[1], r1) - s.qid.begin();
    const long long at = 1000;
    const int32_t nr = r1 - r0;
    std::vector<long long> off((size_t)nr + 1, -7), want_off((size_t)nr + 1, 0);
    std::vector<uint32_t> win((size_t)std::max<long long>(hi - lo, 1), 0xdeadbeefu), want_win(win.size(), 0xdeadbeefu);
    for (int32_t r = r0; r <= r1; ++r) want_off[(size_t)(r - r0)] = at + (std::lower_bound(s.qid.begin() + lo, s.qid.begin() + hi, r) - (s.qid.begin() + lo));
    for (long long i = lo; i < hi; ++i) {
        const uint32_t first = (uint32_t)(s.qs[(size_t)i] / reso), last1 = s.qe[(size_t)i] > 0 ? (uint32_t)((s.qe[(size_t)i] - 1) / reso) + 1u : 0u;
        want_win[(size_t)(i - lo)] = last1 > first ? (first | (last1 << 16)) : 0u;
    }
    const WindowDiv div(reso);
    bool good = true;
    for (int t = 0; t < T; ++t) good = derive_slice(t, T, s.qid.data(), s.qs.data(), s.qe.data(), lo, hi, r0, r1, div, at, off.data(), win.data()) && good;
    CHECK(good, "derive [%d, %d) T %d", r0, r1, T);
    CHECK(off == want_off, "derive [%d, %d) T %d: offsets", r0, r1, T);
    CHECK(win == want_win, "derive [%d, %d) T %d: window records", r0, r1, T);
}

static void check_derive_slice()
{
    const int32_t reso = 50;
    for (Shape shape : {kEven, kGaps, kOneRead}) {
        const Stream s = make_stream(1000, 1, shape, reso);
        for (int T : {1, 3}) {
            check_derive(s, 0, 1000, reso, T);
            check_derive(s, 137, 611, reso, T);
            check_derive(s, 2, 3, reso, T);              // (kGaps: a chunk without records)
        }
    }
    // what sends the job to the one-piece pass
    const WindowDiv div(reso);
    struct { const char *what; int32_t qid[4], qs[4], qe[4]; int32_t r0, r1; } bad[] = {
        {"a negative coordinate", {0, 1, 2, 3}, {0, -1, 0, 0}, {60, 60, 60, 60}, 0, 4},
        {"a window index of 65536", {0, 1, 2, 3}, {0, 0, 0, 0}, {60, 60, 65535 * reso + 1, 60}, 0, 4},
        {"an id stepping back", {0, 2, 1, 3}, {0, 0, 0, 0}, {60, 60, 60, 60}, 0, 4},
        {"an id at r1", {0, 1, 2, 4}, {0, 0, 0, 0}, {60, 60, 60, 60}, 0, 4},
        {"an id below r0", {2, 3, 0, 3}, {0, 0, 0, 0}, {60, 60, 60, 60}, 2, 4},
        {"a first id below r0", {0, 2, 3, 3}, {0, 0, 0, 0}, {60, 60, 60, 60}, 2, 4}};
    for (auto &b : bad)
        for (int T : {1, 3}) {
            long long off[8] = {};
            uint32_t win[4] = {};
            bool good = true;
            for (int t = 0; t < T; ++t) good = derive_slice(t, T, b.qid, b.qs, b.qe, 0, 4, b.r0, b.r1, div, 0, off, win) && good;
            CHECK(!good, "%s (T %d) went through", b.what, T);
        }
    const int32_t q[4] = {0, 1, 2, 3}, a[4] = {0, 0, 0, 0}, e[4] = {60, 60, 65535 * reso, 60};
    long long off[8] = {};
    uint32_t win[4] = {};
    CHECK(derive_slice(0, 1, q, a, e, 0, 4, 0, 4, div, 0, off, win) && win[2] == (65535u << 16), "a window index of 65535: %08x", win[2]);
}

// ---- the same plans as before the planner was lifted out of run_multi_impl: the literals are what that code gave for these inputs
struct LiteralCase { const char *what; int32_t n_reads; int n_seg; Shape shape; bool grouped; int want; bool ramp, d4; std::vector<long long> flat; };

static std::vector<long long> flatten(const std::vector<ChunkPlan> &plan, int n_seg)
{
    std::vector<long long> f;
    for (const ChunkPlan &cp : plan) {
        f.push_back(cp.r0); f.push_back(cp.r1); f.push_back(cp.n_rec); f.push_back(cp.win_lo);
        for (int g = 0; g < n_seg; ++g) { f.push_back(cp.piece[g].lo); f.push_back(cp.piece[g].hi); }
    }
    return f;
}

static std::vector<LiteralCase> literal_cases()
{
    return {
        {"columns, 2 runs, 5 chunks", 1000, 2, kEven, false, 5, false, false, {
             0, 200, 800, 0, 0, 400, 2000, 2400, 200, 400, 800, 0, 400, 800, 2400, 2800, 400, 600, 800, 0, 800, 1200,
             2800, 3200, 600, 800, 800, 0, 1200, 1600, 3200, 3600, 800, 1000, 800, 0, 1600, 2000, 3600, 4000}},
        {"columns, 2 runs, 23 chunks, ramp", 1000, 2, kEven, false, 23, true, false, {
             0, 23, 91, 0, 0, 46, 2000, 2045, 23, 69, 185, 0, 46, 137, 2045, 2139, 69, 114, 180, 0, 137, 227, 2139,
             2229, 114, 159, 180, 0, 227, 317, 2229, 2319, 159, 205, 184, 0, 317, 410, 2319, 2410, 205, 250, 180, 0,
             410, 500, 2410, 2500, 250, 296, 183, 0, 500, 590, 2500, 2593, 296, 341, 180, 0, 590, 680, 2593, 2683, 341,
             387, 182, 0, 680, 772, 2683, 2773, 387, 433, 186, 0, 772, 866, 2773, 2865, 433, 478, 180, 0, 866, 956,
             2865, 2955, 478, 523, 180, 0, 956, 1046, 2955, 3045, 523, 569, 185, 0, 1046, 1137, 3045, 3139, 569, 614,
             180, 0, 1137, 1227, 3139, 3229, 614, 659, 180, 0, 1227, 1317, 3229, 3319, 659, 705, 184, 0, 1317, 1410,
             3319, 3410, 705, 750, 180, 0, 1410, 1500, 3410, 3500, 750, 796, 183, 0, 1500, 1590, 3500, 3593, 796, 841,
             180, 0, 1590, 1680, 3593, 3683, 841, 887, 182, 0, 1680, 1772, 3683, 3773, 887, 933, 186, 0, 1772, 1866,
             3773, 3865, 933, 978, 180, 0, 1866, 1956, 3865, 3955, 978, 1000, 89, 0, 1956, 2000, 3955, 4000}},
        {"grouped, 4 runs, 5 chunks", 1000, 4, kGaps, true, 5, false, false, {
             0, 200, 536, 0, 0, 135, 669, 800, 1332, 1469, 1999, 2132, 200, 401, 537, 0, 135, 269, 800, 935, 1469, 1600,
             2132, 2269, 401, 599, 527, 0, 269, 400, 935, 1069, 1600, 1732, 2269, 2399, 599, 800, 536, 0, 400, 535,
             1069, 1200, 1732, 1869, 2399, 2532, 800, 1000, 529, 0, 535, 669, 1200, 1332, 1869, 1999, 2532, 2665}},
        {"columns, 1 run, 5 chunks, delta4", 1000, 1, kEven, false, 5, false, true, {
             0, 202, 402, 0, 0, 402, 202, 401, 398, 61116, 402, 800, 401, 604, 407, 121956, 800, 1207, 604, 800, 393,
             183736, 1207, 1600, 800, 1000, 400, 240424, 1600, 2000}},
        {"grouped, 2 runs, 23 chunks, delta4", 1000, 2, kGaps, true, 23, false, true, {
             0, 48, 62, 0, 0, 32, 669, 699, 48, 89, 58, 14288, 32, 60, 699, 729, 89, 133, 55, 25356, 60, 89, 729, 755,
             133, 177, 60, 37256, 89, 119, 755, 785, 177, 219, 57, 51264, 119, 149, 785, 812, 219, 268, 63, 63208, 149,
             179, 812, 845, 268, 311, 60, 78672, 179, 209, 845, 875, 311, 352, 51, 90784, 209, 235, 875, 900, 352, 396,
             60, 102364, 235, 265, 900, 930, 396, 435, 54, 116300, 265, 290, 930, 959, 435, 479, 60, 127880, 290, 320,
             959, 989, 479, 530, 66, 142512, 320, 355, 989, 1020, 530, 566, 49, 158464, 355, 379, 1020, 1045, 566, 610,
             57, 170240, 379, 409, 1045, 1072, 610, 653, 60, 184128, 409, 439, 1072, 1102, 653, 695, 54, 198556, 439,
             465, 1102, 1130, 695, 745, 66, 210780, 465, 499, 1130, 1162, 745, 787, 54, 225876, 499, 525, 1162, 1190,
             787, 827, 56, 237144, 525, 552, 1190, 1219, 827, 870, 58, 250676, 552, 580, 1219, 1249, 870, 915, 60,
             263304, 580, 610, 1249, 1279, 915, 960, 60, 277976, 610, 640, 1279, 1309, 960, 1000, 52, 293712, 640, 669,
             1309, 1332}},
        {"columns, 1 run, 5 reads, 5 chunks", 5, 1, kEven, false, 5, false, false, {
             0, 2, 2, 0, 0, 2, 2, 3, 4, 0, 2, 6, 3, 5, 4, 0, 6, 10}},
    };
}

static void check_literals(bool print)
{
    for (const LiteralCase &lc : literal_cases()) {
        const Stream s = make_stream(lc.n_reads, lc.n_seg, lc.shape, 50);
        const HostInput in = lc.grouped ? s.grouped() : s.columns();
        const std::vector<long long> got = flatten(plan_chunks(in, s.seg, lc.n_seg, lc.want, lc.ramp, lc.d4, 50), lc.n_seg);
        if (print) {
            printf("%s:", lc.what);
            for (long long v : got) printf(" %lld,", v);
            printf("\n");
        } else CHECK(got == lc.flat, "%s: the plan is not the one kept here (%zu values, %zu kept)", lc.what, got.size(), lc.flat.size());
    }
}

int main(int argc, char **argv)
{
    const bool print = argc > 1 && !strcmp(argv[1], "--print");
    if (!print) {
        check_window_div();
        check_guess_segments();
        check_plan_invariants();
        check_d4_moves();
        check_place_jobs();
        check_derive_slice();
    }
    check_literals(print);
    if (g_failed) { fprintf(stderr, "pipeline_plan_check: %d checks failed\n", g_failed); return 1; }
    if (!print) printf("pipeline_plan_check: ok\n");
    return 0;
}
